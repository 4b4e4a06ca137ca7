// pplie-build: precise
// epnp.hip -- batched EPnP (camera pose from N >= 4 matches of 3-D points and pixels; reference pypose/module/pnp.py) in ONE launch:
// points [B, N, 3], pixels [B, N, 2], K [B, 3, 3] (or one shared matrix: stride 0)  ->  SE3 rows [B, 7].  No global workspace.
// (precise: the divisions and square roots here are fp64 and off the bandwidth path.)
//
// The arithmetic of one problem is pnp_math.h's Solver, written against a context; this file supplies the two contexts.
//
//   WAVES = 1 (N < kPnpWideN): one 64-lane wavefront per problem, four problems per 256-lane workgroup.  Lanes run over the points
//   (the first point of a lane stays in registers, so N <= 64 reads memory once; larger N is strided by 64), the sums of a pass go
//   through the DPP prefix of dpp.h, lane 63 leaves the totals in the wave's slice of LDS.  A wavefront executes in lockstep and its
//   LDS operations complete in order, so the path holds no __syncthreads: a compiler-level barrier is all a "sync" is.
//
//   WAVES = 4: one workgroup per problem.  Each wave reduces its share by DPP, the four partial rows cross LDS, wave 0 runs the
//   12 x 12 Jacobi on the shared A and V while the others wait at the barrier that publishes the null vectors.
//
// Per problem the LDS holds A and V (12 x 12 each), the 6 rotations of a Jacobi round, the totals of a pass and the four null
// vectors: 396 doubles, plus 4 x 40 partials in the wide variant.  The small dense stages (3 x 3 Jacobi and SVD, the 6 x k solves,
// Gauss-Newton on the betas) are computed by every lane from those shared numbers: no broadcast, no divergence.
#include <hip/hip_runtime.h>

#include "dpp.h"
#include "pnp_math.h"
#include "pplie.h"

namespace pplie {

enum { kPnpBlock = 256, kPnpShared = 144 + 144 + 12 + pnp::kPnpRed + 48, kPnpWideN = 256 };

__device__ __forceinline__ void pnp_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int WAVES> struct PnpContext {
  double *A, *V, *rot, *red, *nv, *part;
  int tid;                                                  // among the 64 * WAVES lanes of the problem
  __device__ __forceinline__ PnpContext(double* lds, double* partials, int t)
      : A(lds), V(lds + 144), rot(lds + 288), red(lds + 300), nv(lds + 300 + pnp::kPnpRed), part(partials), tid(t) {}
  __device__ __forceinline__ int lane() const { return tid; }
  __device__ __forceinline__ int nl() const { return 64 * WAVES; }
  __device__ __forceinline__ bool dense() const { return tid < 64; }
  __device__ __forceinline__ int dlane() const { return tid; }
  __device__ __forceinline__ int dn() const { return 64; }
  __device__ __forceinline__ void dsync() { pnp_wave_sync(); }
  __device__ __forceinline__ void sync() {
    if (WAVES == 1) pnp_wave_sync(); else __syncthreads();
  }
  __device__ __forceinline__ void reduce(const double* v, int n) {
    if (WAVES == 1) {
      pnp_wave_sync();                                       // every lane is done with the previous totals
      for (int i = 0; i < n; ++i) {
        const double s = wave_total63<double>(v[i]);
        if (tid == 63) red[i] = s;
      }
      pnp_wave_sync();
    } else {
      const int w = tid >> 6;
      for (int i = 0; i < n; ++i) {
        const double s = wave_total63<double>(v[i]);
        if ((tid & 63) == 63) part[w * pnp::kPnpRed + i] = s;
      }
      __syncthreads();                                       // the partials are there, and nobody still reads the old totals
      if (tid < n) {
        double s = part[tid];
        for (int k = 1; k < WAVES; ++k) s += part[k * pnp::kPnpRed + tid];
        red[tid] = s;
      }
      __syncthreads();
    }
  }
};

template <class T> struct PnpArgs {
  const T* points; const T* pixels; const T* K;
  T* pose;
  int64_t B, N, kstride;                                    // kstride: elements between intrinsic matrices (9, or 0 when shared)
  int refine_steps;
};

template <class T, int WAVES>
__global__ void __launch_bounds__(kPnpBlock)
epnp_kernel(PnpArgs<T> a) {
  constexpr int kProblems = WAVES == 1 ? kPnpBlock / 64 : 1;
  __shared__ double lds[kProblems * kPnpShared];
  __shared__ double partials[WAVES == 1 ? 1 : WAVES * pnp::kPnpRed];
  const int slot = WAVES == 1 ? threadIdx.x >> 6 : 0, tid = WAVES == 1 ? threadIdx.x & 63 : threadIdx.x;
  const int64_t b = (int64_t)blockIdx.x * kProblems + slot;
  if (b >= a.B) return;                                      // (a whole wave of the narrow variant: it meets no barrier)
  PnpContext<WAVES> cx(lds + slot * kPnpShared, partials, tid);
  pnp::Solver<T, PnpContext<WAVES>> solver(cx, a.points + b * a.N * 3, a.pixels + b * a.N * 2, a.K + b * a.kstride, a.N);
  double pose[7];
  // a cloud thinner than 32 ulp of its inputs against its length is flat as far as the inputs can tell: no third control point
  const double ulp = sizeof(T) == 4 ? 1.1920928955078125e-07 : 2.220446049250313e-16;
  solver.solve(a.refine_steps, (32 * ulp) * (32 * ulp), pose);
  if (tid == 0)
    for (int i = 0; i < 7; ++i) a.pose[b * 7 + i] = T(pose[i]);
}

template <class T>
int launch_epnp(const void* points, const void* pixels, const void* K, int64_t kstride, void* pose, int64_t B, int64_t N, int refine_steps,
                void* stream) {
  if (B < 0 || N < 4 || refine_steps < 0 || (kstride != 0 && kstride != 9) || N >= (int64_t(1) << 31) || B >= (int64_t(1) << 31))
    return PPLIE_EBADARG;
  if (B == 0) return PPLIE_OK;
  if (!points || !pixels || !K || !pose) return PPLIE_EBADARG;
  PnpArgs<T> a;
  a.points = static_cast<const T*>(points); a.pixels = static_cast<const T*>(pixels); a.K = static_cast<const T*>(K);
  a.pose = static_cast<T*>(pose); a.B = B; a.N = N; a.kstride = kstride; a.refine_steps = refine_steps;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (N < kPnpWideN) {
    hipLaunchKernelGGL((epnp_kernel<T, 1>), dim3((unsigned)((B + 3) / 4)), dim3(kPnpBlock), 0, st, a);
  } else {
    hipLaunchKernelGGL((epnp_kernel<T, 4>), dim3((unsigned)B), dim3(kPnpBlock), 0, st, a);
  }
  return hipGetLastError() == hipSuccess ? PPLIE_OK : PPLIE_ELAUNCH;
}

}  // namespace pplie

extern "C" int pplie_epnp_f32(const void* points, const void* pixels, const void* K, int64_t kstride, void* pose, int64_t B, int64_t N,
                              int refine_steps, void* stream) {
  return pplie::launch_epnp<float>(points, pixels, K, kstride, pose, B, N, refine_steps, stream);
}
extern "C" int pplie_epnp_f64(const void* points, const void* pixels, const void* K, int64_t kstride, void* pose, int64_t B, int64_t N,
                              int refine_steps, void* stream) {
  return pplie::launch_epnp<double>(points, pixels, K, kstride, pose, B, N, refine_steps, stream);
}

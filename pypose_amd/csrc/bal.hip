// pplie-build: no-packed-fp32
// bal.hip -- Snavely / BAL reprojection residual of one (intrinsics, camera pose, point, observed pixel) tuple with its
// closed-form Jacobian blocks for all three optimised operands (arithmetic: bal_math.h; the model of examples/ba.py and of
// the reference's examples/module/ba/bundle_adjustment.py:16-43).  Four operands in, three gradients out: more than the
// uniform row ABI carries (PPLIE_ROW_ARGS: 3 in, 2 out), so these kernels have entry points of their own:
//
//   pplie_se3_bal_fwd (K [n,3], X [n,7], p [n,3], uv [n,2] | NULL) -> r [n,2]
//   pplie_se3_bal_lin (K, X, p, uv | NULL)                         -> r [n,2], J [n,24]
//   pplie_bal_vjp     (J [n,24], g [n,2])                          -> gK [n,3], gX [n,7] (7th component 0), gp [n,3]
//
// K = (f, k1, k2); J = [n, 2, 12] row-major, each residual row [dK (3) | dpose (6, left tangent) | dpoint (3)]; a NULL uv
// is zero (r is the projection).  The depth division is the model's plain division: no homo2cart clamp (bal_math.h).
//
// Design.  One observation per lane.  The operand rows are 12 / 28 / 12 / 8 B in and 8 / 96 B out (fp32): none is a
// multiple of 16 B, so a lane never touches global memory for its own row.  A workgroup owns a tile of TILE consecutive
// observations; the tile's byte range of every operand is contiguous and (TILE a multiple of 4, base pointers 16-byte
// aligned) starts and ends on 16 B, so it moves HBM <-> LDS as cooperative dwordx4 accesses -- rowmap.h's slab helpers,
// which also carry the ragged last tile and unaligned bases element by element.  Lanes read their rows from LDS, compute
// in registers and write r and J back into LDS; the tile leaves as dwordx4 slab stores.
//   LDS banks: the 3- and 7-wide rows have odd pitches (conflict-free ds_read_b32); the 2-wide rows move as one b64 per
//   lane; the 24-wide J row would put 64 lanes on 8 banks (gcd(24, 64) = 8), so J sits in LDS at a pitch of 25 scalars
//   (fp64: 50 dwords, 32 distinct even banks per half-wave of b64) and the slab copy re-indexes: a 16 B global vector
//   never straddles a J row (24 % 4 == 0), it is gathered from / scattered to one LDS row.
//   J is written with ordinary stores: the assembly that follows reads it straight back.
//   No matrix instructions: the work is 2x2, 2x3 and 3x3 products private to a row, nothing is shared across lanes.
// Algorithmic bytes per observation (fp32): lin 60 read + 104 written, fwd 60 + 8, vjp 104 + 52.
#include "rowmap.h"
#include "bal_math.h"

namespace pplie {

// Tile = workgroup size (one observation per lane).  lin: 15 + 2 + 25 = 42 scalars of LDS per row, vjp: 25 + 2 + 13 = 40.
// fp32 at 128 rows: 21.0 KB -> 7 workgroups (14 waves) per CU of 160 KB; the pinhole se3_reproj_lin, the same shape of
// kernel at 41 scalars per row, measured fastest at 128 x 1 (reproj.hip).  fp64 at 128 rows: 42 KB -> 3 workgroups (6
// waves) per CU.  fwd: 17 scalars per row, 256 rows = 17 KB (fp32) / 34 KB (fp64).  Expected occupancies, not yet
// revisited against a measurement of these kernels.
constexpr int kBalTile32 = 128;
constexpr int kBalTile64 = 128;
constexpr int kBalFwdTile = 256;
constexpr int kBalJPitch = BAL_JROW + 1;

// J tile between global memory (row pitch 24) and LDS (row pitch 25)
template <class T, int BLOCK, int TILE, bool VEC>
__device__ __forceinline__ void bal_j_g2s(const T* __restrict__ g, T* __restrict__ s, int rows, bool full) {
  const int tid = threadIdx.x;
  if (VEC && full) {
    constexpr int EPV = 16 / (int)sizeof(T);
    constexpr int NV = TILE * BAL_JROW / EPV;
    static_assert(BAL_JROW % EPV == 0 && NV % BLOCK == 0, "a 16 B vector stays inside one J row; whole vectors per lane");
#pragma unroll
    for (int k = 0; k < NV / BLOCK; ++k) {
      const int idx = tid + k * BLOCK, e = idx * EPV, row = e / BAL_JROW;
      const raw16 v = reinterpret_cast<const raw16*>(g)[idx];
      T t[EPV];
      __builtin_memcpy(t, &v, sizeof(v));
#pragma unroll
      for (int c = 0; c < EPV; ++c) s[e + row + c] = t[c];          // row * 25 + (e - row * 24) + c
    }
  } else {
    for (int i = tid; i < rows * BAL_JROW; i += BLOCK) s[i + i / BAL_JROW] = g[i];
  }
}
template <class T, int BLOCK, int TILE, bool VEC>
__device__ __forceinline__ void bal_j_s2g(const T* __restrict__ s, T* __restrict__ g, int rows, bool full) {
  const int tid = threadIdx.x;
  if (VEC && full) {
    constexpr int EPV = 16 / (int)sizeof(T);
    constexpr int NV = TILE * BAL_JROW / EPV;
    static_assert(BAL_JROW % EPV == 0 && NV % BLOCK == 0, "a 16 B vector stays inside one J row; whole vectors per lane");
#pragma unroll
    for (int k = 0; k < NV / BLOCK; ++k) {
      const int idx = tid + k * BLOCK, e = idx * EPV, row = e / BAL_JROW;
      T t[EPV];
#pragma unroll
      for (int c = 0; c < EPV; ++c) t[c] = s[e + row + c];
      raw16 v;
      __builtin_memcpy(&v, t, sizeof(v));
      reinterpret_cast<raw16*>(g)[idx] = v;
    }
  } else {
    for (int i = tid; i < rows * BAL_JROW; i += BLOCK) g[i] = s[i + i / BAL_JROW];
  }
}

// residual (LIN: and Jacobian blocks) of a tile of observations per workgroup
template <class T, int BLOCK, bool VEC, bool LIN, bool HAS_UV>
__global__ void __launch_bounds__(BLOCK)
bal_kernel(const T* __restrict__ K, const T* __restrict__ X, const T* __restrict__ p, const T* __restrict__ uv,
           T* __restrict__ r, T* __restrict__ J, int64_t n) {
  constexpr int TILE = BLOCK;
  constexpr int UW = HAS_UV ? 2 : 0, JP = LIN ? kBalJPitch : 0;
  constexpr int OFF_X = TILE * 3, OFF_P = OFF_X + TILE * 7, OFF_UV = OFF_P + TILE * 3, OFF_R = OFF_UV + TILE * UW,
                OFF_J = OFF_R + TILE * 2, TOTAL = OFF_J + TILE * JP;
  static_assert(TILE % 4 == 0, "every slab starts on 16 B");
  __shared__ __attribute__((aligned(16))) T lds[TOTAL];

  const int64_t ntiles = (n + TILE - 1) / TILE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * TILE;
    const int64_t left = n - row0;
    const bool full = left >= TILE;
    const int rows = full ? TILE : (int)left;

    slab_g2s<T, BLOCK, TILE * 3, VEC>(K + row0 * 3, lds, rows * 3, full);
    slab_g2s<T, BLOCK, TILE * 7, VEC>(X + row0 * 7, lds + OFF_X, rows * 7, full);
    slab_g2s<T, BLOCK, TILE * 3, VEC>(p + row0 * 3, lds + OFF_P, rows * 3, full);
    if constexpr (HAS_UV) slab_g2s<T, BLOCK, TILE * 2, VEC>(uv + row0 * 2, lds + OFF_UV, rows * 2, full);
    __syncthreads();

    const int row = threadIdx.x;
    if (row < rows) {
      T k[3], x[7], pt[3], u[2], res[2], jac[LIN ? BAL_JROW : 1];
      row_ld<3>(lds + row * 3, k);
      row_ld<7>(lds + OFF_X + row * 7, x);
      row_ld<3>(lds + OFF_P + row * 3, pt);
      if constexpr (HAS_UV) row_ld<2>(lds + OFF_UV + row * 2, u);
      se3_bal_core<T>(k, x, pt, HAS_UV ? u : nullptr, res, LIN ? jac : nullptr);
      row_st<2>(lds + OFF_R + row * 2, res);
      if constexpr (LIN) {
#pragma unroll
        for (int c = 0; c < BAL_JROW; ++c) lds[OFF_J + row * JP + c] = jac[c];
      }
    }
    __syncthreads();

    slab_s2g<T, BLOCK, TILE * 2, VEC>(lds + OFF_R, r + row0 * 2, rows * 2, full);
    if constexpr (LIN) bal_j_s2g<T, BLOCK, TILE, VEC>(lds + OFF_J, J + row0 * BAL_JROW, rows, full);
    // no third barrier (as rowmap_lds_kernel): the next tile's loads write the input slabs only, which every lane finished
    // reading before the barrier above; the output slabs are rewritten after the next tile's first barrier
  }
}

template <class T, int BLOCK, bool VEC>
__global__ void __launch_bounds__(BLOCK)
bal_vjp_kernel(const T* __restrict__ J, const T* __restrict__ g, T* __restrict__ gK, T* __restrict__ gX, T* __restrict__ gp,
               int64_t n) {
  constexpr int TILE = BLOCK;
  constexpr int OFF_G = TILE * kBalJPitch, OFF_K = OFF_G + TILE * 2, OFF_X = OFF_K + TILE * 3, OFF_P = OFF_X + TILE * 7,
                TOTAL = OFF_P + TILE * 3;
  static_assert(TILE % 4 == 0, "every slab starts on 16 B");
  __shared__ __attribute__((aligned(16))) T lds[TOTAL];

  const int64_t ntiles = (n + TILE - 1) / TILE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * TILE;
    const int64_t left = n - row0;
    const bool full = left >= TILE;
    const int rows = full ? TILE : (int)left;

    bal_j_g2s<T, BLOCK, TILE, VEC>(J + row0 * BAL_JROW, lds, rows, full);
    slab_g2s<T, BLOCK, TILE * 2, VEC>(g + row0 * 2, lds + OFF_G, rows * 2, full);
    __syncthreads();

    const int row = threadIdx.x;
    if (row < rows) {
      T jac[BAL_JROW], cot[2], ok[3], ox[7], op[3];
#pragma unroll
      for (int c = 0; c < BAL_JROW; ++c) jac[c] = lds[row * kBalJPitch + c];
      row_ld<2>(lds + OFF_G + row * 2, cot);
      bal_vjp<T>(jac, cot, ok, ox, op);
      row_st<3>(lds + OFF_K + row * 3, ok);
      row_st<7>(lds + OFF_X + row * 7, ox);
      row_st<3>(lds + OFF_P + row * 3, op);
    }
    __syncthreads();

    slab_s2g<T, BLOCK, TILE * 3, VEC>(lds + OFF_K, gK + row0 * 3, rows * 3, full);
    slab_s2g<T, BLOCK, TILE * 7, VEC>(lds + OFF_X, gX + row0 * 7, rows * 7, full);
    slab_s2g<T, BLOCK, TILE * 3, VEC>(lds + OFF_P, gp + row0 * 3, rows * 3, full);
  }
}

inline int bal_grid(int64_t n, int tile) {
  const int64_t ntiles = (n + tile - 1) / tile;
  return (int)(ntiles < kGridCap ? ntiles : kGridCap);
}

template <class T, int BLOCK, bool LIN>
int launch_bal(const void* K, const void* X, const void* p, const void* uv, void* r, void* J, int64_t n, void* stream) {
  if (n < 0) return PPLIE_EBADARG;
  if (n == 0) return PPLIE_OK;
  if (!K || !X || !p || !r || (LIN && !J)) return PPLIE_EBADARG;
  const bool vec = aligned16(K) && aligned16(X) && aligned16(p) && aligned16(uv) && aligned16(r) && (!LIN || aligned16(J));
  const dim3 grid(bal_grid(n, BLOCK)), block(BLOCK);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const T *k = static_cast<const T*>(K), *x = static_cast<const T*>(X), *pt = static_cast<const T*>(p), *u = static_cast<const T*>(uv);
  T *ro = static_cast<T*>(r), *jo = static_cast<T*>(J);
  if (vec && uv) hipLaunchKernelGGL((bal_kernel<T, BLOCK, true, LIN, true>), grid, block, 0, st, k, x, pt, u, ro, jo, n);
  else if (vec) hipLaunchKernelGGL((bal_kernel<T, BLOCK, true, LIN, false>), grid, block, 0, st, k, x, pt, u, ro, jo, n);
  else if (uv) hipLaunchKernelGGL((bal_kernel<T, BLOCK, false, LIN, true>), grid, block, 0, st, k, x, pt, u, ro, jo, n);
  else hipLaunchKernelGGL((bal_kernel<T, BLOCK, false, LIN, false>), grid, block, 0, st, k, x, pt, u, ro, jo, n);
  return hipGetLastError() == hipSuccess ? PPLIE_OK : PPLIE_ELAUNCH;
}

template <class T, int BLOCK>
int launch_bal_vjp(const void* J, const void* g, void* gK, void* gX, void* gp, int64_t n, void* stream) {
  if (n < 0) return PPLIE_EBADARG;
  if (n == 0) return PPLIE_OK;
  if (!J || !g || !gK || !gX || !gp) return PPLIE_EBADARG;
  const bool vec = aligned16(J) && aligned16(g) && aligned16(gK) && aligned16(gX) && aligned16(gp);
  const dim3 grid(bal_grid(n, BLOCK)), block(BLOCK);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const T *j = static_cast<const T*>(J), *c = static_cast<const T*>(g);
  T *ok = static_cast<T*>(gK), *ox = static_cast<T*>(gX), *op = static_cast<T*>(gp);
  if (vec) hipLaunchKernelGGL((bal_vjp_kernel<T, BLOCK, true>), grid, block, 0, st, j, c, ok, ox, op, n);
  else hipLaunchKernelGGL((bal_vjp_kernel<T, BLOCK, false>), grid, block, 0, st, j, c, ok, ox, op, n);
  return hipGetLastError() == hipSuccess ? PPLIE_OK : PPLIE_ELAUNCH;
}

}  // namespace pplie

extern "C" int pplie_se3_bal_fwd_f32(const void* K, const void* X, const void* p, const void* uv, void* r, int64_t n, void* stream) {
  return pplie::launch_bal<float, pplie::kBalFwdTile, false>(K, X, p, uv, r, nullptr, n, stream);
}
extern "C" int pplie_se3_bal_fwd_f64(const void* K, const void* X, const void* p, const void* uv, void* r, int64_t n, void* stream) {
  return pplie::launch_bal<double, pplie::kBalFwdTile, false>(K, X, p, uv, r, nullptr, n, stream);
}
extern "C" int pplie_se3_bal_lin_f32(const void* K, const void* X, const void* p, const void* uv, void* r, void* J, int64_t n,
                                     void* stream) {
  return pplie::launch_bal<float, pplie::kBalTile32, true>(K, X, p, uv, r, J, n, stream);
}
extern "C" int pplie_se3_bal_lin_f64(const void* K, const void* X, const void* p, const void* uv, void* r, void* J, int64_t n,
                                     void* stream) {
  return pplie::launch_bal<double, pplie::kBalTile64, true>(K, X, p, uv, r, J, n, stream);
}
extern "C" int pplie_bal_vjp_f32(const void* J, const void* g, void* gK, void* gX, void* gp, int64_t n, void* stream) {
  return pplie::launch_bal_vjp<float, pplie::kBalTile32>(J, g, gK, gX, gp, n, stream);
}
extern "C" int pplie_bal_vjp_f64(const void* J, const void* g, void* gK, void* gX, void* gp, int64_t n, void* stream) {
  return pplie::launch_bal_vjp<double, pplie::kBalTile64>(J, g, gK, gX, gp, n, stream);
}

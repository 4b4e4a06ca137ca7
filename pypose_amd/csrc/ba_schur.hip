// pplie-build: no-packed-fp32
// ba_schur.hip -- bundle adjustment with the points eliminated: PCG on the reduced camera system S = U - W V^-1 W^T applied
// implicitly (optim/multigraph.py SchurPCG route).  Observation e couples camera c(e) (kept, MB = 6 | 9 unknowns: pose, or
// intrinsics + pose) and point p(e) (eliminated, 3 unknowns) through Jc_e [2, MB] and Jp_e [2, 3]:
//
//   V_p = sum_{e in p} Jp^T Jp + diag(shift_p)          Pi t = t - Jp V^-1 Jp^T t   (on per-observation 2-vectors)
//   S x = Jc^T Pi Jc x + shift_c o x                    b_S  = -Jc^T Pi r           x_p = -V_p^-1 sum_{e in p} Jp^T (r + Jc x_c)
//
// Layout.  pplie_ba_schur_pack gathers the caller's edge-major slot blocks once per linearisation into a point-major copy
// JP [E, 2 (MB + 3)] = rows [Jc_0 | Jp_0 | Jc_1 | Jp_1] (MB = 9: 24 scalars, 96 B in fp32) with the residual rP [E, 2], and a
// camera-major copy JC [E, 2 MB] (sorted by camera, then point).  A lane gathers one source row into LDS, the tile leaves as
// dwordx4 slabs (rowmap.h).  The index plan (sort orders, CSR pointers, camP / posPC / posCP / ptC, work items) is the caller's,
// built once per index structure.
//
// Point pass (pplie_ba_schur_point; every iteration with MODE 0).  Lanes own observations, whole points own lane groups: a
// point with n <= 64 observations gets G = the next power of two lanes, 64 / G points share a wavefront (the plan sorts the
// points by G) and sum_e Jp^T t is an xor butterfly inside the group -- every lane of the group ends with the same bits.  A
// point with n > 64 owns a workgroup: chunks of 256 observations, butterfly per wavefront, the four partials through LDS in
// fixed order, chunk sums added in chunk order, then a second sweep that applies V^-1 (the single-chunk case keeps its rows
// in registers).  No atomics on data; run-to-run bit-identical.  The camera vector (A + beta B: the search direction
// z + beta p is formed on the fly) is staged in LDS by each (persistent) workgroup when Nc MB scalars fit, else gathered.
//   MODE 0: t = Jc x -> u = Pi t at the observation's camera-major position     MODE 1: t = r (b_S)
//   MODE 2: t = r + Jc x -> x_p (back-substitution)                             MODE 3: V_p, closed-form inverse -> Vinv [Np, 6]
// Camera pass (pplie_ba_schur_cam).  One workgroup per work item (camera, <= PPLIE_BA_SCHUR_CCHUNK camera-major observations,
// contiguous reads); a camera of several items is finished by the item that arrives last (integer counter; it adds the parts
// in item order).  The finisher writes p_c = z_c + beta p_c, q_c = sum Jc^T u + shift_c o p_c and p_c . q_c; the camera that
// arrives last adds the Nc dot products in index order and leaves alpha = rho / p.q.
// Step (pplie_ba_schur_step).  16 lanes per camera: x += alpha p, r -= alpha q, z = S_cc^-1 r (block rows by shuffles), r.z and
// r.r per workgroup; the last workgroup adds them in order and leaves rho, beta and |r|^2 in hist[k].  Three launches per
// iteration, every scalar on the device, no host synchronisation; a linear chain (capturable).
// Set-up (pplie_ba_schur_blocks): one workgroup per camera accumulates U_c and, per run of observations of one point,
// G = sum Jc^T Jp and - G V^-1 G^T (exactly S's diagonal block also when a camera sees a point twice), then MB lanes solve one
// column each of the inverse (chol.h).
#include "rowmap.h"
#include "chol.h"

namespace pplie {

enum { PPLIE_EUNSUPPORTED = -4 };
constexpr int kSchurBlock = 256;      // workgroup; also the chunk of the long-point path
constexpr int kSchurPackTile = 128;
constexpr int kSchurMaxKept = 3;
constexpr int kSchurStageBytes = 32 << 10;
enum { SCAL_RHO = 0, SCAL_ALPHA = 1, SCAL_BETA = 2 };

template <class T> __device__ __forceinline__ T pp_fma(T a, T b, T c) { return __builtin_fma(a, b, c); }
template <> __device__ __forceinline__ float pp_fma<float>(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

template <class T> __device__ __forceinline__ T vload(const T* p) { return *reinterpret_cast<const volatile T*>(p); }

// all 64 lanes end with the same bits (a + b is commutative at every level)
template <class T, int N> __device__ __forceinline__ void wave_allsum(T* v, int width) {
  for (int o = width >> 1; o > 0; o >>= 1) {
#pragma unroll
    for (int r = 0; r < N; ++r) v[r] += __shfl_xor(v[r], o, 64);
  }
}

// ---------------------------------------------------------------------------------------------------------------- pack
struct SchurSlots {
  const void* J[kSchurMaxKept];
  int m[kSchurMaxKept];
  int n;
};

template <class T, int MB, bool WITHP>
__global__ void __launch_bounds__(kSchurPackTile)
schur_pack_kernel(SchurSlots kept, const T* __restrict__ Jp, const T* __restrict__ R, const int* __restrict__ perm,
                  T* __restrict__ out, T* __restrict__ rout, int64_t E, int vec) {
  constexpr int TILE = kSchurPackTile, HW = MB + (WITHP ? 3 : 0), RW = 2 * HW;
  __shared__ __attribute__((aligned(16))) T lds[TILE * RW];
  const int64_t ntiles = (E + TILE - 1) / TILE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * TILE;
    const int64_t left = E - row0;
    const bool full = left >= TILE;
    const int rows = full ? TILE : (int)left;
    const int k = threadIdx.x;
    if (k < rows) {
      const int64_t e = perm[row0 + k];
      T* d = lds + k * RW;
      int off = 0;
      for (int s = 0; s < kept.n; ++s) {
        const int m = kept.m[s];
        const T* J = static_cast<const T*>(kept.J[s]) + e * 2 * m;
        for (int i = 0; i < m; ++i) {
          d[off + i] = J[i];
          d[HW + off + i] = J[m + i];
        }
        off += m;
      }
      if constexpr (WITHP) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          d[MB + i] = Jp[e * 6 + i];
          d[HW + MB + i] = Jp[e * 6 + 3 + i];
        }
        rout[(row0 + k) * 2] = R[e * 2];
        rout[(row0 + k) * 2 + 1] = R[e * 2 + 1];
      }
    }
    __syncthreads();
    if (vec) slab_s2g<T, TILE, TILE * RW, true>(lds, out + row0 * RW, rows * RW, full);
    else slab_s2g<T, TILE, TILE * RW, false>(lds, out + row0 * RW, rows * RW, full);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------- point pass
template <class T> struct SchurPointArgs {
  const T* JP; const T* rP; const int* camP; const int* posPC; const int* ptrP;
  const int* plist; const int* witems; int nW; const int* litems; int nL;
  const T* A; const T* B; const T* scal;
  T* Vinv; const T* shiftP; T* u; T* xp;
  int Nc; int stage;
};

// y = V^-1 s for the packed symmetric (00 01 02 11 12 22)
template <class T> __device__ __forceinline__ void sym3_apply(const T* v, const T* s, T* y) {
  y[0] = v[0] * s[0] + v[1] * s[1] + v[2] * s[2];
  y[1] = v[1] * s[0] + v[3] * s[1] + v[4] * s[2];
  y[2] = v[2] * s[0] + v[4] * s[1] + v[5] * s[2];
}

// one observation: its row, t (MODE 0: Jc x, 1: r, 2: r + Jc x) and w = Jp^T t (MODE 3: the packed Jp^T Jp)
template <class T, int MB, int MODE>
__device__ __forceinline__ void schur_obs(const SchurPointArgs<T>& a, const T* xs, T beta, int k, bool act, T* row, T* t, T* w) {
  constexpr int HW = MB + 3, RW = 2 * HW, NR = MODE == 3 ? 6 : 3;
  t[0] = t[1] = T(0);
#pragma unroll
  for (int r = 0; r < NR; ++r) w[r] = T(0);
  if (!act) return;
  row_ld<RW>(a.JP + (int64_t)k * RW, row);
  const T *p0 = row + MB, *p1 = row + HW + MB;
  if constexpr (MODE == 3) {
    w[0] = p0[0] * p0[0] + p1[0] * p1[0];
    w[1] = p0[0] * p0[1] + p1[0] * p1[1];
    w[2] = p0[0] * p0[2] + p1[0] * p1[2];
    w[3] = p0[1] * p0[1] + p1[1] * p1[1];
    w[4] = p0[1] * p0[2] + p1[1] * p1[2];
    w[5] = p0[2] * p0[2] + p1[2] * p1[2];
  } else {
    if constexpr (MODE == 1 || MODE == 2) {
      t[0] = a.rP[(int64_t)k * 2];
      t[1] = a.rP[(int64_t)k * 2 + 1];
    }
    if constexpr (MODE == 0 || MODE == 2) {
      const int64_t c = (int64_t)a.camP[k] * MB;
#pragma unroll
      for (int i = 0; i < MB; ++i) {
        const T xv = a.stage ? xs[c + i] : (a.B ? pp_fma(beta, a.B[c + i], a.A[c + i]) : a.A[c + i]);
        t[0] += row[i] * xv;
        t[1] += row[HW + i] * xv;
      }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = p0[i] * t[0] + p1[i] * t[1];
  }
}

template <class T, int MB, int MODE>
__device__ __forceinline__ void schur_finish(const SchurPointArgs<T>& a, int p, int k, bool act, bool head, const T* row, const T* t,
                                             const T* s) {
  constexpr int HW = MB + 3;
  if constexpr (MODE == 0 || MODE == 1) {
    if (act) {
      T vi[6], v[3];
#pragma unroll
      for (int i = 0; i < 6; ++i) vi[i] = a.Vinv[(int64_t)p * 6 + i];
      sym3_apply(vi, s, v);
      const T *p0 = row + MB, *p1 = row + HW + MB;
      const int64_t pos = a.posPC[k];
      a.u[pos * 2] = t[0] - (p0[0] * v[0] + p0[1] * v[1] + p0[2] * v[2]);
      a.u[pos * 2 + 1] = t[1] - (p1[0] * v[0] + p1[1] * v[1] + p1[2] * v[2]);
    }
  } else if constexpr (MODE == 2) {
    if (head) {
      T vi[6], v[3];
#pragma unroll
      for (int i = 0; i < 6; ++i) vi[i] = a.Vinv[(int64_t)p * 6 + i];
      sym3_apply(vi, s, v);
#pragma unroll
      for (int i = 0; i < 3; ++i) a.xp[(int64_t)p * 3 + i] = -v[i];
    }
  } else {
    if (head) {          // closed-form inverse of the SPD 3x3 block (cofactors / determinant)
      const T a00 = s[0] + a.shiftP[(int64_t)p * 3], a01 = s[1], a02 = s[2], a11 = s[3] + a.shiftP[(int64_t)p * 3 + 1], a12 = s[4],
              a22 = s[5] + a.shiftP[(int64_t)p * 3 + 2];
      const T c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
      const T c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
      const T idet = T(1) / (a00 * c00 + a01 * c01 + a02 * c02);
      T* o = a.Vinv + (int64_t)p * 6;
      o[0] = c00 * idet; o[1] = c01 * idet; o[2] = c02 * idet; o[3] = c11 * idet; o[4] = c12 * idet; o[5] = c22 * idet;
    }
  }
}

template <class T, int MB, int MODE>
__global__ void __launch_bounds__(kSchurBlock)
schur_point_kernel(SchurPointArgs<T> a) {
  constexpr int RW = 2 * (MB + 3), NR = MODE == 3 ? 6 : 3;
  extern __shared__ __attribute__((aligned(16))) unsigned char schur_smem[];
  T* xs = reinterpret_cast<T*>(schur_smem);
  __shared__ T part[4][NR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  T beta = T(0);
  if constexpr (MODE == 0 || MODE == 2) {
    if (a.B) beta = a.scal[SCAL_BETA];
    if (a.stage) {
      for (int i = tid; i < a.Nc * MB; i += kSchurBlock) xs[i] = a.B ? pp_fma(beta, a.B[i], a.A[i]) : a.A[i];
      __syncthreads();
    }
  }
  const int nWG = (a.nW + 3) / 4;
  T row[RW], t[2], w[NR];
  for (int wg = blockIdx.x; wg < nWG + a.nL; wg += gridDim.x) {
    if (wg < nWG) {                                   // four wavefronts, each with 64 / G whole points of G lanes
      const int wi = wg * 4 + wave;
      if (wi < a.nW) {
        const int lg = a.witems[wi * 3], off = a.witems[wi * 3 + 1], cnt = a.witems[wi * 3 + 2];
        const int g = lane >> lg, j = lane & ((1 << lg) - 1);
        const bool valid = g < cnt;
        const int p = valid ? a.plist[off + g] : 0;
        const int beg = valid ? a.ptrP[p] : 0, n = valid ? a.ptrP[p + 1] - beg : 0;
        const bool act = j < n;
        const int k = beg + j;
        schur_obs<T, MB, MODE>(a, xs, beta, k, act, row, t, w);
        wave_allsum<T, NR>(w, 1 << lg);
        schur_finish<T, MB, MODE>(a, p, k, act, valid && j == 0, row, t, w);
      }
    } else {                                          // one point with more than 64 observations per workgroup
      const int p = a.litems[wg - nWG];
      const int beg = a.ptrP[p], end = a.ptrP[p + 1];
      const int nch = (end - beg + kSchurBlock - 1) / kSchurBlock;
      T s[NR];
#pragma unroll
      for (int r = 0; r < NR; ++r) s[r] = T(0);
      for (int ch = 0; ch < nch; ++ch) {
        const int k = beg + ch * kSchurBlock + tid;
        schur_obs<T, MB, MODE>(a, xs, beta, k, k < end, row, t, w);
        wave_allsum<T, NR>(w, 64);
        if (lane == 0) {
#pragma unroll
          for (int r = 0; r < NR; ++r) part[wave][r] = w[r];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < NR; ++r) s[r] += (part[0][r] + part[1][r]) + (part[2][r] + part[3][r]);
        __syncthreads();
      }
      if constexpr (MODE >= 2) {
        schur_finish<T, MB, MODE>(a, p, beg, false, tid == 0, row, t, s);
      } else {
        for (int ch = 0; ch < nch; ++ch) {
          const int k = beg + ch * kSchurBlock + tid;
          if (nch > 1) schur_obs<T, MB, MODE>(a, xs, beta, k, k < end, row, t, w);
          schur_finish<T, MB, MODE>(a, p, k, k < end, false, row, t, s);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- camera pass
template <class T> struct SchurCamArgs {
  const T* JC; const T* u; const int* citems; int nI; const int* cfirst; const int* cnitems;
  T* part; int* ccnt; int* gcnt;
  const T* A; T* B; const T* shiftC; T* q; T* dots; T* scal;
  int Nc; int neg;
};

template <class T, int MB>
__global__ void __launch_bounds__(kSchurBlock)
schur_cam_kernel(SchurCamArgs<T> a) {
  __shared__ T red[4][MB];
  __shared__ T red2[4];
  __shared__ int last_item, last_cam;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int item = blockIdx.x;
  const int c = a.citems[item * 3], beg = a.citems[item * 3 + 1], end = a.citems[item * 3 + 2];
  T acc[MB];
#pragma unroll
  for (int i = 0; i < MB; ++i) acc[i] = T(0);
  for (int j = beg + tid; j < end; j += kSchurBlock) {
    T row[2 * MB];
    row_ld<2 * MB>(a.JC + (int64_t)j * 2 * MB, row);
    const T u0 = a.u[(int64_t)j * 2], u1 = a.u[(int64_t)j * 2 + 1];
#pragma unroll
    for (int i = 0; i < MB; ++i) acc[i] += row[i] * u0 + row[MB + i] * u1;
  }
  wave_allsum<T, MB>(acc, 64);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < MB; ++i) red[wave][i] = acc[i];
  }
  __syncthreads();
  T mine = T(0);
  if (tid < MB) mine = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
  const int ni = a.cnitems[c];
  if (ni > 1) {                                        // several items: the one that arrives last adds the parts in item order
    if (tid < MB) {
      a.part[(int64_t)item * MB + tid] = mine;
      __threadfence();
    }
    __syncthreads();
    if (tid == 0) last_item = atomicAdd(&a.ccnt[c], 1) == ni - 1;
    __syncthreads();
    if (!last_item) return;
    __threadfence();
    if (tid < MB) {
      mine = T(0);
      const int f = a.cfirst[c];
      for (int m = 0; m < ni; ++m) mine += vload(a.part + (int64_t)(f + m) * MB + tid);
    }
    if (tid == 0) a.ccnt[c] = 0;
  }
  T pi = T(0), qi = T(0);
  if (tid < MB) {
    const int64_t idx = (int64_t)c * MB + tid;
    pi = a.A[idx];
    if (a.B) {
      pi = pp_fma(a.scal[SCAL_BETA], a.B[idx], pi);
      a.B[idx] = pi;
    }
    qi = a.neg ? -mine : pp_fma(a.shiftC[idx], pi, mine);
    a.q[idx] = qi;
  }
  if (wave == 0) {
    T d[1] = {pi * qi};
    wave_allsum<T, 1>(d, 16);
    if (tid == 0) {
      a.dots[c] = d[0];
      __threadfence();
      last_cam = atomicAdd(a.gcnt, 1) == a.Nc - 1;
    }
  }
  __syncthreads();
  if (!last_cam) return;
  __threadfence();                                     // the camera that arrives last: p.q in index order, alpha
  T v[1] = {T(0)};
  for (int i = tid; i < a.Nc; i += kSchurBlock) v[0] += vload(a.dots + i);
  wave_allsum<T, 1>(v, 64);
  if (lane == 0) red2[wave] = v[0];
  __syncthreads();
  if (tid == 0) {
    const T pq = (red2[0] + red2[1]) + (red2[2] + red2[3]);
    a.scal[SCAL_ALPHA] = pq != T(0) ? a.scal[SCAL_RHO] / pq : T(0);
    *a.gcnt = 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------- step
template <class T> struct SchurStepArgs {
  T* x; T* r; T* p; const T* q; T* z; const T* Minv; const T* b; T* scal; T* wpart; int* gcnt; T* hist;
  int k; int Nc; int init;
};

template <class T, int MB>
__global__ void __launch_bounds__(kSchurBlock)
schur_step_kernel(SchurStepArgs<T> a) {
  __shared__ T red[4][2];
  __shared__ int last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = blockIdx.x * (kSchurBlock / 16) + (tid >> 4), i = tid & 15;
  const bool act = c < a.Nc && i < MB;
  const int64_t idx = (int64_t)c * MB + i;
  const T alpha = a.scal[SCAL_ALPHA];
  T ri = T(0);
  if (act) {
    if (a.init) {
      ri = a.b[idx];
      a.x[idx] = T(0);
      a.p[idx] = T(0);
    } else {
      ri = pp_fma(-alpha, a.q[idx], a.r[idx]);
      a.x[idx] = pp_fma(alpha, a.p[idx], a.x[idx]);
    }
    a.r[idx] = ri;
  }
  T zi = T(0);
#pragma unroll
  for (int j = 0; j < MB; ++j) {
    const T rj = __shfl(ri, j, 16);
    if (act) zi += a.Minv[idx * MB + j] * rj;
  }
  if (act) a.z[idx] = zi;
  T d[2] = {ri * zi, ri * ri};
  wave_allsum<T, 2>(d, 64);
  if (lane == 0) {
    red[wave][0] = d[0];
    red[wave][1] = d[1];
  }
  __syncthreads();
  if (tid == 0) {
    a.wpart[blockIdx.x * 2] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
    a.wpart[blockIdx.x * 2 + 1] = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
    __threadfence();
    last = atomicAdd(a.gcnt, 1) == (int)gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  __threadfence();                                     // the workgroup that arrives last: r.z and r.r in workgroup order
  T v[2] = {T(0), T(0)};
  for (int g = tid; g < (int)gridDim.x; g += kSchurBlock) {
    v[0] += vload(a.wpart + g * 2);
    v[1] += vload(a.wpart + g * 2 + 1);
  }
  wave_allsum<T, 2>(v, 64);
  __syncthreads();
  if (lane == 0) {
    red[wave][0] = v[0];
    red[wave][1] = v[1];
  }
  __syncthreads();
  if (tid == 0) {
    const T rho_new = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
    const T rr = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
    const T rho = a.scal[SCAL_RHO];
    a.scal[SCAL_BETA] = (a.init || rho == T(0)) ? T(0) : rho_new / rho;
    a.scal[SCAL_RHO] = rho_new;
    a.hist[a.k] = rr;
    *a.gcnt = 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------- S_cc
template <class T> struct SchurBlockArgs {
  const T* JP; const int* posCP; const int* ptC; const int* ptrC; const T* Vinv; const T* shiftC; T* Scc; T* Minv;
  int schur;
};

template <class T, int MB>
__global__ void __launch_bounds__(kSchurBlock)
schur_blocks_kernel(SchurBlockArgs<T> a) {
  constexpr int HW = MB + 3, RW = 2 * HW, NS = MB * (MB + 1) / 2;
  __shared__ T red[4][NS];
  __shared__ T Sf[MB * MB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = blockIdx.x;
  const int beg = a.ptrC[c], end = a.ptrC[c + 1];
  T acc[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) acc[i] = T(0);
  for (int j = beg + tid; j < end; j += kSchurBlock) {
    const int pt = a.ptC[j];
    if (j > beg && a.ptC[j - 1] == pt) continue;      // the head of a run of observations of one point owns the run
    T G[MB][3];
#pragma unroll
    for (int i = 0; i < MB; ++i) G[i][0] = G[i][1] = G[i][2] = T(0);
    for (int jj = j; jj < end && a.ptC[jj] == pt; ++jj) {
      T row[RW];
      row_ld<RW>(a.JP + (int64_t)a.posCP[jj] * RW, row);
      int n = 0;
#pragma unroll
      for (int i = 0; i < MB; ++i) {
#pragma unroll
        for (int l = i; l < MB; ++l) acc[n++] += row[i] * row[l] + row[HW + i] * row[HW + l];
#pragma unroll
        for (int m = 0; m < 3; ++m) G[i][m] += row[i] * row[MB + m] + row[HW + i] * row[HW + MB + m];
      }
    }
    if (a.schur) {
      T vi[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) vi[i] = a.Vinv[(int64_t)pt * 6 + i];
      int n = 0;
#pragma unroll
      for (int i = 0; i < MB; ++i) {
        T h[3];
        sym3_apply(vi, G[i], h);
#pragma unroll
        for (int l = i; l < MB; ++l) acc[n++] -= h[0] * G[l][0] + h[1] * G[l][1] + h[2] * G[l][2];
      }
    }
  }
  wave_allsum<T, NS>(acc, 64);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < NS; ++i) red[wave][i] = acc[i];
  }
  __syncthreads();
  if (tid < NS) {
    int i = 0, first = 0;
    while (tid >= first + (MB - i)) {
      first += MB - i;
      ++i;
    }
    const int l = i + (tid - first);
    T v = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    if (i == l) v += a.shiftC[(int64_t)c * MB + i];
    Sf[i * MB + l] = v;
    Sf[l * MB + i] = v;
  }
  __syncthreads();
  if (tid < MB * MB) a.Scc[(int64_t)c * MB * MB + tid] = Sf[tid];
  if (tid < MB) {                                      // column tid of the inverse
    T A[MB * MB], g[MB], x[MB];
#pragma unroll
    for (int i = 0; i < MB * MB; ++i) A[i] = Sf[i];
#pragma unroll
    for (int i = 0; i < MB; ++i) g[i] = (i == tid) ? T(-1) : T(0);
    Op_chol_solve<T, MB>::apply(A, g, nullptr, x, nullptr);
#pragma unroll
    for (int i = 0; i < MB; ++i) a.Minv[(int64_t)c * MB * MB + i * MB + tid] = x[i];
  }
}

// ---------------------------------------------------------------------------------------------------------------- launchers
inline int schur_status() { return hipGetLastError() == hipSuccess ? PPLIE_OK : PPLIE_ELAUNCH; }

template <class T, int MB>
int schur_pack(const SchurSlots& kept, const void* Jp, const void* R, const void* permP, const void* permC, void* JP, void* rP, void* JC,
               int64_t E, hipStream_t st) {
  const int64_t ntiles = (E + kSchurPackTile - 1) / kSchurPackTile;
  const dim3 grid((unsigned)(ntiles < 65536 ? ntiles : 65536)), block(kSchurPackTile);
  const int vec = aligned16(JP) && aligned16(JC);
  hipLaunchKernelGGL((schur_pack_kernel<T, MB, true>), grid, block, 0, st, kept, static_cast<const T*>(Jp), static_cast<const T*>(R),
                     static_cast<const int*>(permP), static_cast<T*>(JP), static_cast<T*>(rP), E, vec);
  hipLaunchKernelGGL((schur_pack_kernel<T, MB, false>), grid, block, 0, st, kept, static_cast<const T*>(nullptr),
                     static_cast<const T*>(nullptr), static_cast<const int*>(permC), static_cast<T*>(JC), static_cast<T*>(nullptr), E, vec);
  return schur_status();
}

template <class T>
int launch_schur_pack(int nkept, const void* const* Jk, const int* mk, const void* Jp, const void* R, const void* permP, const void* permC,
                      void* JP, void* rP, void* JC, int64_t E, int dr, int ma, void* stream) {
  if (E < 0 || nkept < 1 || !Jk || !mk) return PPLIE_EBADARG;
  if (dr != 2 || ma != 3 || nkept > kSchurMaxKept) return PPLIE_EUNSUPPORTED;
  SchurSlots kept;
  int mb = 0;
  kept.n = nkept;
  for (int s = 0; s < kSchurMaxKept; ++s) {
    kept.J[s] = s < nkept ? Jk[s] : nullptr;
    kept.m[s] = s < nkept ? mk[s] : 0;
    if (s < nkept && (mk[s] < 1 || !Jk[s])) return PPLIE_EBADARG;
    mb += kept.m[s];
  }
  if (mb != 6 && mb != 9) return PPLIE_EUNSUPPORTED;
  if (E == 0) return PPLIE_OK;
  if (E >= (int64_t(1) << 31) / 24) return PPLIE_ECAPACITY;      // int32 positions
  if (!Jp || !R || !permP || !permC || !JP || !rP || !JC) return PPLIE_EBADARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return mb == 6 ? schur_pack<T, 6>(kept, Jp, R, permP, permC, JP, rP, JC, E, st) : schur_pack<T, 9>(kept, Jp, R, permP, permC, JP, rP, JC, E, st);
}

template <class T, int MB, int MODE>
int schur_point(const SchurPointArgs<T>& a, hipStream_t st) {
  const int nwg = (a.nW + 3) / 4 + a.nL;
  if (nwg == 0) return PPLIE_OK;
  const size_t lds = a.stage ? (size_t)a.Nc * MB * sizeof(T) : 0;
  hipLaunchKernelGGL((schur_point_kernel<T, MB, MODE>), dim3(nwg < 2048 ? nwg : 2048), dim3(kSchurBlock), lds, st, a);
  return schur_status();
}

template <class T>
int launch_schur_point(int mode, int mb, const void* JP, const void* rP, const void* camP, const void* posPC, const void* ptrP,
                       const void* plist, const void* witems, int nW, const void* litems, int nL, const void* A, const void* B,
                       const void* scal, void* Vinv, const void* shiftP, void* u, void* xp, int Nc, void* stream) {
  if (mb != 6 && mb != 9) return PPLIE_EUNSUPPORTED;
  if (mode < 0 || mode > 3 || nW < 0 || nL < 0 || Nc < 0) return PPLIE_EBADARG;
  if (!JP || !ptrP || !Vinv || (nW && (!plist || !witems)) || (nL && !litems)) return PPLIE_EBADARG;
  if ((mode == 0 || mode == 2) && (!A || !camP || (B && !scal))) return PPLIE_EBADARG;
  if ((mode == 1 || mode == 2) && !rP) return PPLIE_EBADARG;
  if ((mode <= 1 && (!u || !posPC)) || (mode == 2 && !xp) || (mode == 3 && !shiftP)) return PPLIE_EBADARG;
  SchurPointArgs<T> a;
  a.JP = static_cast<const T*>(JP); a.rP = static_cast<const T*>(rP); a.camP = static_cast<const int*>(camP);
  a.posPC = static_cast<const int*>(posPC); a.ptrP = static_cast<const int*>(ptrP); a.plist = static_cast<const int*>(plist);
  a.witems = static_cast<const int*>(witems); a.nW = nW; a.litems = static_cast<const int*>(litems); a.nL = nL;
  a.A = static_cast<const T*>(A); a.B = static_cast<const T*>(B); a.scal = static_cast<const T*>(scal);
  a.Vinv = static_cast<T*>(Vinv); a.shiftP = static_cast<const T*>(shiftP); a.u = static_cast<T*>(u); a.xp = static_cast<T*>(xp);
  a.Nc = Nc;
  a.stage = (mode == 0 || mode == 2) && Nc > 0 && (size_t)Nc * mb * sizeof(T) <= (size_t)kSchurStageBytes;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define PPLIE_SCHUR_POINT(MB) \
  switch (mode) { case 0: return schur_point<T, MB, 0>(a, st); case 1: return schur_point<T, MB, 1>(a, st); \
                  case 2: return schur_point<T, MB, 2>(a, st); default: return schur_point<T, MB, 3>(a, st); }
  if (mb == 6) PPLIE_SCHUR_POINT(6)
  PPLIE_SCHUR_POINT(9)
#undef PPLIE_SCHUR_POINT
}

template <class T>
int launch_schur_cam(int mb, const void* JC, const void* u, const void* citems, int nI, const void* cfirst, const void* cnitems, void* part,
                     void* ccnt, void* gcnt, const void* A, void* B, const void* shiftC, void* q, void* dots, void* scal, int Nc, int neg,
                     void* stream) {
  if (mb != 6 && mb != 9) return PPLIE_EUNSUPPORTED;
  if (Nc < 0 || nI < Nc) return PPLIE_EBADARG;         // every camera has at least one (possibly empty) item
  if (Nc == 0) return PPLIE_OK;
  if (!JC || !u || !citems || !cfirst || !cnitems || !part || !ccnt || !gcnt || !A || !q || !dots || !scal || (!neg && !shiftC))
    return PPLIE_EBADARG;
  SchurCamArgs<T> a;
  a.JC = static_cast<const T*>(JC); a.u = static_cast<const T*>(u); a.citems = static_cast<const int*>(citems); a.nI = nI;
  a.cfirst = static_cast<const int*>(cfirst); a.cnitems = static_cast<const int*>(cnitems); a.part = static_cast<T*>(part);
  a.ccnt = static_cast<int*>(ccnt); a.gcnt = static_cast<int*>(gcnt); a.A = static_cast<const T*>(A); a.B = static_cast<T*>(B);
  a.shiftC = static_cast<const T*>(shiftC); a.q = static_cast<T*>(q); a.dots = static_cast<T*>(dots); a.scal = static_cast<T*>(scal);
  a.Nc = Nc; a.neg = neg;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (mb == 6) hipLaunchKernelGGL((schur_cam_kernel<T, 6>), dim3(nI), dim3(kSchurBlock), 0, st, a);
  else hipLaunchKernelGGL((schur_cam_kernel<T, 9>), dim3(nI), dim3(kSchurBlock), 0, st, a);
  return schur_status();
}

template <class T>
int launch_schur_step(int mb, void* x, void* r, void* p, const void* q, void* z, const void* Minv, const void* b, void* scal, void* wpart,
                      void* gcnt, void* hist, int k, int Nc, int init, void* stream) {
  if (mb != 6 && mb != 9) return PPLIE_EUNSUPPORTED;
  if (Nc < 0 || k < 0) return PPLIE_EBADARG;
  if (Nc == 0) return PPLIE_OK;
  if (!x || !r || !p || !z || !Minv || !scal || !wpart || !gcnt || !hist || (init ? !b : !q)) return PPLIE_EBADARG;
  SchurStepArgs<T> a;
  a.x = static_cast<T*>(x); a.r = static_cast<T*>(r); a.p = static_cast<T*>(p); a.q = static_cast<const T*>(q); a.z = static_cast<T*>(z);
  a.Minv = static_cast<const T*>(Minv); a.b = static_cast<const T*>(b); a.scal = static_cast<T*>(scal); a.wpart = static_cast<T*>(wpart);
  a.gcnt = static_cast<int*>(gcnt); a.hist = static_cast<T*>(hist); a.k = k; a.Nc = Nc; a.init = init;
  const int per = kSchurBlock / 16;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (mb == 6) hipLaunchKernelGGL((schur_step_kernel<T, 6>), dim3((Nc + per - 1) / per), dim3(kSchurBlock), 0, st, a);
  else hipLaunchKernelGGL((schur_step_kernel<T, 9>), dim3((Nc + per - 1) / per), dim3(kSchurBlock), 0, st, a);
  return schur_status();
}

template <class T>
int launch_schur_blocks(int mb, const void* JP, const void* posCP, const void* ptC, const void* ptrC, const void* Vinv, const void* shiftC,
                        void* Scc, void* Minv, int Nc, int schur, void* stream) {
  if (mb != 6 && mb != 9) return PPLIE_EUNSUPPORTED;
  if (Nc < 0) return PPLIE_EBADARG;
  if (Nc == 0) return PPLIE_OK;
  if (!JP || !posCP || !ptC || !ptrC || !Vinv || !shiftC || !Scc || !Minv) return PPLIE_EBADARG;
  SchurBlockArgs<T> a;
  a.JP = static_cast<const T*>(JP); a.posCP = static_cast<const int*>(posCP); a.ptC = static_cast<const int*>(ptC);
  a.ptrC = static_cast<const int*>(ptrC); a.Vinv = static_cast<const T*>(Vinv); a.shiftC = static_cast<const T*>(shiftC);
  a.Scc = static_cast<T*>(Scc); a.Minv = static_cast<T*>(Minv); a.schur = schur;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (mb == 6) hipLaunchKernelGGL((schur_blocks_kernel<T, 6>), dim3(Nc), dim3(kSchurBlock), 0, st, a);
  else hipLaunchKernelGGL((schur_blocks_kernel<T, 9>), dim3(Nc), dim3(kSchurBlock), 0, st, a);
  return schur_status();
}

}  // namespace pplie

#define PPLIE_BA_SCHUR_ENTRIES(SFX, T)                                                                                                  \
  extern "C" int pplie_ba_schur_pack_##SFX(int nkept, const void* const* Jk, const int* mk, const void* Jp, const void* R,              \
                                           const void* permP, const void* permC, void* JP, void* rP, void* JC, int64_t E, int dr,      \
                                           int ma, void* stream) {                                                                      \
    return pplie::launch_schur_pack<T>(nkept, Jk, mk, Jp, R, permP, permC, JP, rP, JC, E, dr, ma, stream);                              \
  }                                                                                                                                     \
  extern "C" int pplie_ba_schur_point_##SFX(int mode, int mb, const void* JP, const void* rP, const void* camP, const void* posPC,      \
                                            const void* ptrP, const void* plist, const void* witems, int nW, const void* litems,       \
                                            int nL, const void* A, const void* B, const void* scal, void* Vinv, const void* shiftP,    \
                                            void* u, void* xp, int Nc, void* stream) {                                                  \
    return pplie::launch_schur_point<T>(mode, mb, JP, rP, camP, posPC, ptrP, plist, witems, nW, litems, nL, A, B, scal, Vinv, shiftP,   \
                                        u, xp, Nc, stream);                                                                             \
  }                                                                                                                                     \
  extern "C" int pplie_ba_schur_cam_##SFX(int mb, const void* JC, const void* u, const void* citems, int nI, const void* cfirst,        \
                                          const void* cnitems, void* part, void* ccnt, void* gcnt, const void* A, void* B,             \
                                          const void* shiftC, void* q, void* dots, void* scal, int Nc, int neg, void* stream) {        \
    return pplie::launch_schur_cam<T>(mb, JC, u, citems, nI, cfirst, cnitems, part, ccnt, gcnt, A, B, shiftC, q, dots, scal, Nc, neg,   \
                                      stream);                                                                                          \
  }                                                                                                                                     \
  extern "C" int pplie_ba_schur_step_##SFX(int mb, void* x, void* r, void* p, const void* q, void* z, const void* Minv, const void* b,  \
                                           void* scal, void* wpart, void* gcnt, void* hist, int k, int Nc, int init, void* stream) {   \
    return pplie::launch_schur_step<T>(mb, x, r, p, q, z, Minv, b, scal, wpart, gcnt, hist, k, Nc, init, stream);                       \
  }                                                                                                                                     \
  extern "C" int pplie_ba_schur_blocks_##SFX(int mb, const void* JP, const void* posCP, const void* ptC, const void* ptrC,              \
                                             const void* Vinv, const void* shiftC, void* Scc, void* Minv, int Nc, int schur,           \
                                             void* stream) {                                                                            \
    return pplie::launch_schur_blocks<T>(mb, JP, posCP, ptC, ptrC, Vinv, shiftC, Scc, Minv, Nc, schur, stream);                         \
  }

PPLIE_BA_SCHUR_ENTRIES(f32, float)
PPLIE_BA_SCHUR_ENTRIES(f64, double)

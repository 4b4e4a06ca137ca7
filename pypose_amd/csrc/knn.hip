// pplie-build: no-packed-fp32
// pplie-build: precise
// knn.hip -- brute-force k nearest neighbours of 3-D points (Euclidean, smallest k <= 16) without the [N1, N2] distance matrix,
// and the correspondence statistics of one ICP iteration.  (precise: the one square root per output is correctly rounded; it is
// not on the hot path.)
//
// Partial pass (pplie_knn_partial).  Grid = (tiles of 256 reference points) x (S splits of the neighbour range) x (batch).  One
// lane owns one reference point: its coordinates (optionally moved by the batch element's SE3 row on load) and its sorted best-K
// list (d^2, int32 index) live in registers, the list unrolled for K in {1, 2, 4, 8, 16} >= k.  The workgroup streams its split of
// `nbr` through LDS in tiles of 1024 points: the AoS rows of a tile are one contiguous slab that comes in as lane-contiguous 16-byte
// loads (rowmap.h's way of moving rows) and is scattered into three planes x[], y[], z[].  In the inner loop every lane reads the
// SAME LDS address (a broadcast: no bank conflict) with 16-byte reads, four neighbours per trip; the common trip is 3 subtractions,
// 1 multiplication, 2 fused multiply-adds per pair plus a min tree and one compare per four.  The list is only touched when a
// candidate beats the current K-th.  The next tile's global loads are issued before the current tile is computed on (registers in
// flight, two LDS buffers, one barrier per tile).
//
// Distances are direct differences dx^2 + dy^2 + dz^2.  |a|^2 + |b|^2 - 2 a.b would fit the 16x16x4 MFMA shape exactly, but it loses
// the nearest distances -- the ones that matter -- to cancellation (coordinates ~10 in fp32: d^2 off by ~1e-5 absolute), so matrix
// instructions are deliberately not used.  Candidates are visited in ascending index with a strict <: ties keep the smaller index.
//
// Merge pass (pplie_knn_merge).  One lane per reference point merges its S sorted partial lists in split order (ties again to the
// smaller index) and writes sqrt(d^2) and int64 indices.  With S = 1 the partial pass writes the final outputs itself.
//
// ICP mode of the merge (k = 1, stats != NULL).  The lane gathers its matched neighbour q, re-forms p = T . source and contributes
// to 16 sums per batch element -- sum d, sum p (3), sum q (3), sum q p^T (9) -- carried in fp64 whatever the input type (16 adds per
// point after an N2-long loop), so that sum q p^T - N qbar pbar^T is safe when the centroids are large against the spread.  Order:
// inside the wave by DPP (dpp.h), across the four waves through LDS in wave order, per-workgroup partials to [B, nWG, 16], and the
// workgroup of a batch element that arrives last (int32 counter + __threadfence, the pattern of pplie_ba_schur_cam) adds them in
// workgroup order.  No atomics on data: results are bit-identical from run to run.
#include "knn_tile.h"

namespace pplie {

template <class T> struct KnnPartialArgs {
  const T* ref; const T* nbr; const T* tf;               // tf: SE3 rows [B, 7] or NULL
  T* pd2; int* pidx;                                     // partial lists [B, S, N1, k]
  T* values; int64_t* indices;                           // final outputs [B, N1, k] (S == 1) or NULL
  int64_t N1, N2, ref_bstride, nbr_bstride;              // batch strides in points, 0 = broadcast
  int k, S, vec;
};

template <class T, int K>
__global__ void __launch_bounds__(kKnnBlock)
knn_partial_kernel(KnnPartialArgs<T> a) {
  typedef typename KnnV4<T>::type V4;
  __shared__ __attribute__((aligned(32))) T lds[2][3 * kKnnTile];
  const int tid = threadIdx.x, s = blockIdx.y;
  const int64_t b = blockIdx.z, row = (int64_t)blockIdx.x * kKnnBlock + tid;
  const bool act = row < a.N1;

  T px = T(0), py = T(0), pz = T(0);
  if (act) {
    const T* p = a.ref + (b * a.ref_bstride + row) * 3;
    T q[3] = {p[0], p[1], p[2]};
    if (a.tf) {
      T X[7], o[3];
#pragma unroll
      for (int i = 0; i < 7; ++i) X[i] = a.tf[b * 7 + i];
      se3_act<T>(X, q, o);
      q[0] = o[0]; q[1] = o[1]; q[2] = o[2];
    }
    px = q[0]; py = q[1]; pz = q[2];
  }
  T d[K];
  int id[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    d[i] = knn_inf<T>();
    id[i] = -1;
  }

  const int64_t ntiles = (a.N2 + kKnnTile - 1) / kKnnTile;
  const int t0 = (int)(s * ntiles / a.S), t1 = (int)((s + 1) * ntiles / a.S);      // S <= ntiles: no split is empty
  const T* nb = a.nbr + b * a.nbr_bstride * 3;
  auto full = [&](int t) { return a.vec && (int64_t)(t + 1) * kKnnTile <= a.N2; };
  auto valid = [&](int t) { const int64_t left = a.N2 - (int64_t)t * kKnnTile; return left < kKnnTile ? (int)left : kKnnTile; };

  KnnSlab<T> slab;
  if (full(t0)) {
    knn_fetch<T>(nb + (int64_t)t0 * kKnnTile * 3, slab);
    knn_commit<T>(slab, lds[0]);
  } else {
    knn_load_slow<T>(nb + (int64_t)t0 * kKnnTile * 3, valid(t0), lds[0]);
  }
  __syncthreads();

  for (int t = t0; t < t1; ++t) {
    const int cur = (t - t0) & 1;
    const bool next = t + 1 < t1, nfull = next && full(t + 1);
    if (nfull) knn_fetch<T>(nb + (int64_t)(t + 1) * kKnnTile * 3, slab);            // in flight while this tile is computed on

    const T* sx = lds[cur];
    const T* sy = sx + kKnnTile;
    const T* sz = sy + kKnnTile;
    const int cnt = (valid(t) + 3) & ~3, base = t * kKnnTile;
    V4 nX = *reinterpret_cast<const V4*>(sx), nY = *reinterpret_cast<const V4*>(sy), nZ = *reinterpret_cast<const V4*>(sz);
#pragma unroll 2
    for (int j = 0; j < cnt; j += 4) {
      const V4 X = nX, Y = nY, Z = nZ;
      const int jn = j + 4 < cnt ? j + 4 : j;            // the next four are on their way while these are worked on
      nX = *reinterpret_cast<const V4*>(sx + jn);
      nY = *reinterpret_cast<const V4*>(sy + jn);
      nZ = *reinterpret_cast<const V4*>(sz + jn);
      T dd[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const T dx = X[q] - px, dy = Y[q] - py, dz = Z[q] - pz;
        dd[q] = knn_fma(dz, dz, knn_fma(dy, dy, dx * dx));
      }
      if (knn_min(knn_min(dd[0], dd[1]), knn_min(dd[2], dd[3])) < d[K - 1]) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (dd[q] < d[K - 1]) knn_insert<T, K>(d, id, dd[q], base + j + q);
      }
    }

    if (next) {
      if (nfull) knn_commit<T>(slab, lds[cur ^ 1]);
      else knn_load_slow<T>(nb + (int64_t)(t + 1) * kKnnTile * 3, valid(t + 1), lds[cur ^ 1]);
    }
    __syncthreads();                                     // the other buffer is complete; every lane is done reading this one
  }

  if (!act) return;
  if (a.values) {
    T* v = a.values + (b * a.N1 + row) * a.k;
    int64_t* ix = a.indices + (b * a.N1 + row) * a.k;
#pragma unroll
    for (int j = 0; j < K; ++j)
      if (j < a.k) {
        v[j] = pp_sqrt(d[j]);
        ix[j] = id[j];
      }
  } else {
    const int64_t o = ((b * a.S + s) * a.N1 + row) * a.k;
#pragma unroll
    for (int j = 0; j < K; ++j)
      if (j < a.k) {
        a.pd2[o + j] = d[j];
        a.pidx[o + j] = id[j];
      }
  }
}

template <class T> struct KnnMergeArgs {
  const T* pd2; const int* pidx;                         // [B, S, N1, k]
  T* values; int64_t* indices;                           // [B, N1, k] (may be NULL in ICP mode)
  const T* src; const T* nbr; const T* tf;               // ICP mode: the source cloud, the neighbour cloud, SE3 rows [B, 7] or NULL
  double* wgpart; int* cnt; double* stats;               // [B, nWG, 16], [B], [B, 16]
  int64_t N1, N2, src_bstride, nbr_bstride;
  int k, S;
};

template <class T, int K, bool ICP>
__global__ void __launch_bounds__(kKnnBlock)
knn_merge_kernel(KnnMergeArgs<T> a) {
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.y, row = (int64_t)blockIdx.x * kKnnBlock + tid;
  const bool act = row < a.N1;
  T d[K];
  int id[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    d[i] = knn_inf<T>();
    id[i] = -1;
  }
  if (act) {
    const int64_t o = (b * a.S * a.N1 + row) * a.k;
#pragma unroll
    for (int j = 0; j < K; ++j)
      if (j < a.k) {
        d[j] = a.pd2[o + j];
        id[j] = a.pidx[o + j];
      }
    for (int s = 1; s < a.S; ++s) {                      // split order = ascending index: a tie keeps the entry it already has
      const int64_t os = ((b * a.S + s) * a.N1 + row) * a.k;
      for (int j = 0; j < a.k; ++j) {
        const T c = a.pd2[os + j];
        if (!(c < d[K - 1])) break;                      // the partial list is sorted: nothing behind c gets in either
        knn_insert<T, K>(d, id, c, a.pidx[os + j]);
      }
    }
    if (a.values) {
      T* v = a.values + (b * a.N1 + row) * a.k;
      int64_t* ix = a.indices + (b * a.N1 + row) * a.k;
#pragma unroll
      for (int j = 0; j < K; ++j)
        if (j < a.k) {
          v[j] = pp_sqrt(d[j]);
          ix[j] = id[j];
        }
    }
  }
  if constexpr (ICP) {
    __shared__ double red[kKnnBlock / 64][kKnnStats];
    __shared__ int last;
    double v[kKnnStats];
#pragma unroll
    for (int i = 0; i < kKnnStats; ++i) v[i] = 0.0;
    if (act) {
      const int64_t j = id[0] < 0 ? 0 : id[0];           // (a row of NaNs matches nothing: keep the gather inside the cloud)
      const T* sp = a.src + (b * a.src_bstride + row) * 3;
      const T* qp = a.nbr + (b * a.nbr_bstride + j) * 3;
      T p[3] = {sp[0], sp[1], sp[2]};
      if (a.tf) {
        T X[7], o[3];
#pragma unroll
        for (int i = 0; i < 7; ++i) X[i] = a.tf[b * 7 + i];
        se3_act<T>(X, p, o);
        p[0] = o[0]; p[1] = o[1]; p[2] = o[2];
      }
      v[0] = (double)pp_sqrt(d[0]);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double q = (double)qp[i];
        v[1 + i] = (double)p[i];
        v[4 + i] = q;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[7 + 3 * i + c] = q * (double)p[c];
      }
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < kKnnStats; ++i) {
      const double t = wave_total63<double>(v[i]);       // every lane of the wave takes part; the total is in lane 63
      if (lane == 63) red[wave][i] = t;
    }
    __syncthreads();
    const int nwg = gridDim.x;
    if (tid < kKnnStats) {
      a.wgpart[(b * nwg + blockIdx.x) * kKnnStats + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
      __threadfence();
    }
    __syncthreads();
    if (tid == 0) last = atomicAdd(a.cnt + b, 1) == nwg - 1;
    __syncthreads();
    if (!last) return;
    __threadfence();                                     // the workgroup that arrives last: the partials in workgroup order
    if (tid < kKnnStats) {
      double sum = 0.0;
      for (int g = 0; g < nwg; ++g) sum += knn_vload(a.wgpart + (b * nwg + g) * kKnnStats + tid);
      a.stats[b * kKnnStats + tid] = sum;
    }
    if (tid == 0) a.cnt[b] = 0;
  }
}

inline bool knn_shape_ok(int64_t B, int64_t N1, int64_t N2, int k) {
  return k <= kKnnMaxK && N2 < (int64_t(1) << 31) && N1 < (int64_t(1) << 31) && B <= 65535;
}

template <class T>
int launch_knn_partial(const void* ref, const void* nbr, const void* tf, void* pd2, void* pidx, void* values, void* indices, int64_t B,
                       int64_t N1, int64_t N2, int k, int S, int64_t ref_bstride, int64_t nbr_bstride, void* stream) {
  if (B < 0 || N1 < 0 || N2 < 0 || k < 1 || S < 1 || ref_bstride < 0 || nbr_bstride < 0) return PPLIE_EBADARG;
  if (!knn_shape_ok(B, N1, N2, k)) return PPLIE_EUNSUPPORTED;
  if (k > N2) return PPLIE_EBADARG;
  if (B == 0 || N1 == 0) return PPLIE_OK;
  const int64_t ntiles = (N2 + kKnnTile - 1) / kKnnTile;
  if (S > ntiles || S > 65535) return PPLIE_EBADARG;
  const bool final = values != nullptr;
  if (!ref || !nbr || (final ? (!indices || S != 1) : (!pd2 || !pidx))) return PPLIE_EBADARG;
  KnnPartialArgs<T> a;
  a.ref = static_cast<const T*>(ref); a.nbr = static_cast<const T*>(nbr); a.tf = static_cast<const T*>(tf);
  a.pd2 = static_cast<T*>(pd2); a.pidx = static_cast<int*>(pidx); a.values = static_cast<T*>(values);
  a.indices = static_cast<int64_t*>(indices); a.N1 = N1; a.N2 = N2; a.ref_bstride = ref_bstride; a.nbr_bstride = nbr_bstride;
  a.k = k; a.S = S;
  a.vec = aligned16(nbr) && (nbr_bstride * 3 * (int64_t)sizeof(T)) % 16 == 0;       // every tile slab starts on 16 bytes
  const dim3 grid((unsigned)((N1 + kKnnBlock - 1) / kKnnBlock), (unsigned)S, (unsigned)B), block(kKnnBlock);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  switch (knn_width(k)) {
    case 1: hipLaunchKernelGGL((knn_partial_kernel<T, 1>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((knn_partial_kernel<T, 2>), grid, block, 0, st, a); break;
    case 4: hipLaunchKernelGGL((knn_partial_kernel<T, 4>), grid, block, 0, st, a); break;
    case 8: hipLaunchKernelGGL((knn_partial_kernel<T, 8>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((knn_partial_kernel<T, 16>), grid, block, 0, st, a); break;
  }
  return knn_status();
}

template <class T>
int launch_knn_merge(const void* pd2, const void* pidx, void* values, void* indices, const void* src, const void* nbr, const void* tf,
                     void* wgpart, void* cnt, void* stats, int64_t B, int64_t N1, int64_t N2, int k, int S, int64_t src_bstride,
                     int64_t nbr_bstride, void* stream) {
  if (B < 0 || N1 < 0 || N2 < 0 || k < 1 || S < 1 || src_bstride < 0 || nbr_bstride < 0) return PPLIE_EBADARG;
  if (!knn_shape_ok(B, N1, N2, k)) return PPLIE_EUNSUPPORTED;
  const bool icp = stats != nullptr;
  if (icp && k != 1) return PPLIE_EUNSUPPORTED;
  if (k > N2) return PPLIE_EBADARG;
  if (B == 0 || N1 == 0) return PPLIE_OK;
  if (!pd2 || !pidx || (values ? !indices : !icp) || (icp && (!src || !nbr || !wgpart || !cnt))) return PPLIE_EBADARG;
  KnnMergeArgs<T> a;
  a.pd2 = static_cast<const T*>(pd2); a.pidx = static_cast<const int*>(pidx); a.values = static_cast<T*>(values);
  a.indices = static_cast<int64_t*>(indices); a.src = static_cast<const T*>(src); a.nbr = static_cast<const T*>(nbr);
  a.tf = static_cast<const T*>(tf); a.wgpart = static_cast<double*>(wgpart); a.cnt = static_cast<int*>(cnt);
  a.stats = static_cast<double*>(stats); a.N1 = N1; a.N2 = N2; a.src_bstride = src_bstride; a.nbr_bstride = nbr_bstride;
  a.k = k; a.S = S;
  const dim3 grid((unsigned)((N1 + kKnnBlock - 1) / kKnnBlock), (unsigned)B), block(kKnnBlock);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (icp) {
    hipLaunchKernelGGL((knn_merge_kernel<T, 1, true>), grid, block, 0, st, a);
    return knn_status();
  }
  switch (knn_width(k)) {
    case 1: hipLaunchKernelGGL((knn_merge_kernel<T, 1, false>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((knn_merge_kernel<T, 2, false>), grid, block, 0, st, a); break;
    case 4: hipLaunchKernelGGL((knn_merge_kernel<T, 4, false>), grid, block, 0, st, a); break;
    case 8: hipLaunchKernelGGL((knn_merge_kernel<T, 8, false>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((knn_merge_kernel<T, 16, false>), grid, block, 0, st, a); break;
  }
  return knn_status();
}

}  // namespace pplie

#define PPLIE_KNN_ENTRIES(SFX, T)                                                                                                       \
  extern "C" int pplie_knn_partial_##SFX(const void* ref, const void* nbr, const void* tf, void* pd2, void* pidx, void* values,        \
                                         void* indices, int64_t B, int64_t N1, int64_t N2, int k, int S, int64_t ref_bstride,          \
                                         int64_t nbr_bstride, void* stream) {                                                          \
    return pplie::launch_knn_partial<T>(ref, nbr, tf, pd2, pidx, values, indices, B, N1, N2, k, S, ref_bstride, nbr_bstride, stream);   \
  }                                                                                                                                     \
  extern "C" int pplie_knn_merge_##SFX(const void* pd2, const void* pidx, void* values, void* indices, const void* src,                \
                                       const void* nbr, const void* tf, void* wgpart, void* cnt, void* stats, int64_t B, int64_t N1,   \
                                       int64_t N2, int k, int S, int64_t src_bstride, int64_t nbr_bstride, void* stream) {             \
    return pplie::launch_knn_merge<T>(pd2, pidx, values, indices, src, nbr, tf, wgpart, cnt, stats, B, N1, N2, k, S, src_bstride,       \
                                      nbr_bstride, stream);                                                                             \
  }
PPLIE_KNN_ENTRIES(f32, float)
PPLIE_KNN_ENTRIES(f64, double)

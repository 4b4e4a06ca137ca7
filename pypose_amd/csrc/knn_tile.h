// knn_tile.h -- what the streaming point-cloud kernels share (knn.hip, cloud_filter.hip): the sorted best-K list in registers and
// the loaders that bring a 1024-point tile of a contiguous [N, 3] cloud from HBM into three LDS planes.
#pragma once
#include "rowmap.h"
#include "dpp.h"

namespace pplie {

enum { PPLIE_EUNSUPPORTED = -4 };
constexpr int kKnnBlock = 256;       // reference points per workgroup, one per lane
constexpr int kKnnTile = 1024;       // neighbour points per LDS tile
constexpr int kKnnMaxK = 16;
constexpr int kKnnStats = 16;

template <class T> struct KnnV4 { typedef T __attribute__((ext_vector_type(4))) type; };
template <class T> __device__ __forceinline__ T knn_fma(T a, T b, T c) { return __builtin_fma(a, b, c); }
template <> __device__ __forceinline__ float knn_fma<float>(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
template <class T> __device__ __forceinline__ T knn_min(T a, T b) { return __builtin_fmin(a, b); }
template <> __device__ __forceinline__ float knn_min<float>(float a, float b) { return __builtin_fminf(a, b); }
template <class T> __device__ __forceinline__ T knn_inf() { return T(__builtin_huge_valf()); }
template <class T> __device__ __forceinline__ T knn_vload(const T* p) { return *reinterpret_cast<const volatile T*>(p); }

// sorted insertion of (c, ci) into the ascending list d[0..K-1]; the caller has checked c < d[K-1].  An entry equal to c stays
// in front of it (it was visited earlier, so its index is smaller).
template <class T, int K> __device__ __forceinline__ void knn_insert(T* d, int* id, T c, int ci) {
#pragma unroll
  for (int i = K - 1; i > 0; --i) {
    if (c < d[i - 1]) {
      d[i] = d[i - 1];
      id[i] = id[i - 1];
    } else if (c < d[i]) {
      d[i] = c;
      id[i] = ci;
    }
  }
  if (c < d[0]) {
    d[0] = c;
    id[0] = ci;
  }
}

// the same for candidates that do not arrive in ascending index (knn_grid.hip): the list is ordered by (d^2, index), which is the
// order the ascending visit with a strict < leaves.  The caller has checked (c, ci) < (d[K-1], id[K-1]).
template <class T> __device__ __forceinline__ bool knn_before(T c, int ci, T d, int id) { return c < d || (c == d && ci < id); }
template <class T, int K> __device__ __forceinline__ void knn_insert_lex(T* d, int* id, T c, int ci) {
#pragma unroll
  for (int i = K - 1; i > 0; --i) {
    if (knn_before(c, ci, d[i - 1], id[i - 1])) {
      d[i] = d[i - 1];
      id[i] = id[i - 1];
    } else if (knn_before(c, ci, d[i], id[i])) {
      d[i] = c;
      id[i] = ci;
    }
  }
  if (knn_before(c, ci, d[0], id[0])) {
    d[0] = c;
    id[0] = ci;
  }
}

// minimum over the 64 lanes, valid in lane 63: wave_prefix_add's seven DPP steps with min for + and +inf for 0
template <class T> __device__ __forceinline__ T wave_min63(T v) {
  const T v0 = v, z = knn_inf<T>();
  v = knn_min(dpp_mov<DPP_ROW_SHR1, 0xf, 0xf>(z, v0), v);
  v = knn_min(dpp_mov<DPP_ROW_SHR2, 0xf, 0xf>(z, v0), v);
  v = knn_min(dpp_mov<DPP_ROW_SHR3, 0xf, 0xf>(z, v0), v);
  v = knn_min(dpp_mov<DPP_ROW_SHR4, 0xf, 0xe>(z, v), v);
  v = knn_min(dpp_mov<DPP_ROW_SHR8, 0xf, 0xc>(z, v), v);
  v = knn_min(dpp_mov<DPP_ROW_BCAST15, 0xa, 0xf>(z, v), v);
  v = knn_min(dpp_mov<DPP_ROW_BCAST31, 0xc, 0xf>(z, v), v);
  return v;
}

// ---- a tile of `nbr` from HBM to the three LDS planes
// full && vec: the slab of kKnnTile rows as 16-byte loads, held in registers (knn_fetch) until the previous tile is done with
// (knn_commit).  Otherwise element by element (the ragged last tile of the cloud, or a base that is not 16-byte aligned), with
// the planes padded to a multiple of four points by x = +inf (a distance that never beats a list entry).
template <class T> struct KnnSlab {
  static constexpr int NV = kKnnTile * 3 * (int)sizeof(T) / 16, PER = NV / kKnnBlock, EPV = 16 / (int)sizeof(T);
  raw16 v[PER];
};

template <class T> __device__ __forceinline__ void knn_fetch(const T* __restrict__ g, KnnSlab<T>& r) {
#pragma unroll
  for (int i = 0; i < KnnSlab<T>::PER; ++i) r.v[i] = reinterpret_cast<const raw16*>(g)[threadIdx.x + i * kKnnBlock];
}

template <class T> __device__ __forceinline__ void knn_commit(const KnnSlab<T>& r, T* __restrict__ planes) {
  constexpr int EPV = KnnSlab<T>::EPV;
#pragma unroll
  for (int i = 0; i < KnnSlab<T>::PER; ++i) {
    T e[EPV];
    __builtin_memcpy(e, &r.v[i], 16);
    const int e0 = (threadIdx.x + i * kKnnBlock) * EPV;
#pragma unroll
    for (int c = 0; c < EPV; ++c) {
      const int pt = (e0 + c) / 3, comp = (e0 + c) - 3 * pt;
      planes[comp * kKnnTile + pt] = e[c];
    }
  }
}

template <class T> __device__ __forceinline__ void knn_load_slow(const T* __restrict__ g, int valid, T* __restrict__ planes) {
  for (int i = threadIdx.x; i < valid * 3; i += kKnnBlock) {
    const int pt = i / 3, comp = i - 3 * pt;
    planes[comp * kKnnTile + pt] = g[i];
  }
  const int padded = (valid + 3) & ~3;                   // <= kKnnTile: the tile is a multiple of four
  for (int pt = valid + threadIdx.x; pt < padded; pt += kKnnBlock) {
    planes[pt] = knn_inf<T>();
    planes[kKnnTile + pt] = T(0);
    planes[2 * kKnnTile + pt] = T(0);
  }
}

inline int knn_status() { return hipGetLastError() == hipSuccess ? PPLIE_OK : PPLIE_ELAUNCH; }
inline int knn_width(int k) { return k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : 16; }

}  // namespace pplie

// knn_grid_box.h -- what the kernels that search a KnnIndex share (knn_grid.hip, nbr_grid.hip): the cell arithmetic and the header
// of the uniform grid, the union of the lanes' cell ranges into one workgroup box, the table of the box's runs of the sorted
// planes, and the loaders that bring 1024 points of the concatenated runs from HBM into LDS planes.
#pragma once
#include <climits>

#include "knn_tile.h"

namespace pplie {

constexpr int kGridBlock = 256;
constexpr int kGridMaxAxis = 128;    // cells per axis
constexpr int kGridRuns = 256;       // runs of the box in LDS at a time
constexpr int kGridHdr = 8;          // doubles per header: min (3), h, gx, gy, gz, non-finite flag

// cell of the offset coordinate rel = p - min on an axis of g cells; anything below the grid (and a NaN) goes to cell 0
template <class T> __device__ __forceinline__ int grid_cell(T rel, T h, int g) {
  const T q = rel / h;
  return !(q > T(0)) ? 0 : q >= T(g) ? g - 1 : (int)q;
}

template <class T> struct GridHeader {
  T mn[3], h;
  int g[3];
  __device__ __forceinline__ explicit GridHeader(const double* H) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      mn[c] = (T)H[c];
      g[c] = (int)H[4 + c];
    }
    h = (T)H[3];
  }
};

// The workgroup's box: the union of the open lanes' cell ranges lo[c] .. hi[c] (some lane is open), clamped to the grid of g[]
// cells; unless `first`, at least the box that sbox[] holds from the call before grown by a cell on each side.  Left in sbox[]
// and in blo[], bhi[] of every lane (every lane calls it; barriers inside).  red: [kGridBlock / 64][6] floats.
__device__ __forceinline__ void grid_box_union(bool open, const int* lo, const int* hi, const int* g, bool first, float (*red)[6],
                                               int* sbox, int* blo, int* bhi) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g0 = g[0], g1 = g[1], g2 = g[2];             // (read here: a select between the addresses would pin g[] to scratch)
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    const float w = !open ? knn_inf<float>() : c < 3 ? (float)lo[c] : (float)-hi[c - 3];      // |cells| <= 129: exact
    const float t = wave_min63<float>(w);
    if (lane == 63) red[wave][c] = t;
  }
  __syncthreads();
  if (tid < 6) {
    const int c = tid < 3 ? tid : tid - 3, top = (c == 0 ? g0 : c == 1 ? g1 : g2) - 1;
    const int prev = sbox[tid];                          // (the previous box; not read on the first pass)
    const float m = knn_min(knn_min(red[0][tid], red[1][tid]), knn_min(red[2][tid], red[3][tid]));
    int v = tid < 3 ? (int)m : (int)-m;
    if (tid < 3) {
      if (!first && v > prev - 1) v = prev - 1;
      v = v < 0 ? 0 : v;
    } else {
      if (!first && v < prev + 1) v = prev + 1;
      v = v > top ? top : v;
    }
    sbox[tid] = v;
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    blo[c] = sbox[c];
    bhi[c] = sbox[3 + c];
  }
}

// The runs r0 .. r0 + nr - 1 of the box (one per (y, z): cells blo[0] .. bhi[0] are contiguous in the sorted planes; by = the
// box's extent in y): rbeg[i] = sorted position of the run's first point, rpre[i] = its position in the stream of the
// concatenated runs.  Returns the length of that stream (every lane calls it; barriers inside).  wsum: [kGridBlock / 64].
__device__ __forceinline__ int grid_run_table(const int* __restrict__ starts, int cb, const int* g, const int* blo, const int* bhi,
                                              int by, int r0, int nr, int* rbeg, int* rpre, double* wsum) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int len = 0;
  if (tid < nr) {
    const int r = r0 + tid, zz = blo[2] + r / by, yy = blo[1] + r % by, c0 = cb + (zz * g[1] + yy) * g[0];
    const int s = starts[c0 + blo[0]];
    rbeg[tid] = s;
    len = starts[c0 + bhi[0] + 1] - s;
  }
  const double inc = wave_prefix_add<double>((double)len);            // (integers below 2^31: exact)
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  double off = 0.0;
  for (int u = 0; u < wave; ++u) off += wsum[u];
  if (tid < nr) rpre[tid] = (int)(off + inc) - len;                   // stream position of the run's first point
  const int total = (int)(((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]);
  __syncthreads();
  return total;
}

// Tile t of the stream in registers: four positions per lane, lane-contiguous inside a run, +inf padding behind the end.  IDX:
// with the original index of every point (INT_MAX behind the end).
template <class T, bool IDX> struct GridFetch {
  T x[4], y[4], z[4];
  int id[IDX ? 4 : 1];
};

// stream position -> sorted position: the last run that starts at or before it (runs of length 0 are stepped over)
template <class T, bool IDX>
__device__ __forceinline__ void grid_fetch(int t, int total, int nr, const int* rbeg, const int* rpre, const T* __restrict__ gx,
                                           const T* __restrict__ gy, const T* __restrict__ gz, const int* __restrict__ oidx,
                                           GridFetch<T, IDX>& f) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int v = t * kKnnTile + i * kKnnBlock + (int)threadIdx.x;
    f.x[i] = knn_inf<T>();
    f.y[i] = T(0);
    f.z[i] = T(0);
    if constexpr (IDX) f.id[i] = INT_MAX;
    if (v < total) {
      int r = 0;
#pragma unroll
      for (int step = kGridRuns / 2; step > 0; step >>= 1) {
        const int c = r + step;
        if (c < nr && rpre[c] <= v) r = c;
      }
      const int src = rbeg[r] + (v - rpre[r]);
      f.x[i] = gx[src];
      f.y[i] = gy[src];
      f.z[i] = gz[src];
      if constexpr (IDX) f.id[i] = oidx[src];
    }
  }
}

template <class T, bool IDX>
__device__ __forceinline__ void grid_commit(const GridFetch<T, IDX>& f, T* __restrict__ planes, int* __restrict__ ids) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int v = i * kKnnBlock + (int)threadIdx.x;
    planes[v] = f.x[i];
    planes[kKnnTile + v] = f.y[i];
    planes[2 * kKnnTile + v] = f.z[i];
    if constexpr (IDX) ids[v] = f.id[i];
  }
}

}  // namespace pplie

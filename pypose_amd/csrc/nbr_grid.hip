// pplie-build: no-packed-fp32
// pplie-build: precise
// nbr_grid.hip -- how many points of a cloud lie within a fixed radius of each of its points, through the uniform grid that
// pp.knn_index has built over that cloud (knn_grid.hip): the count that nbr_filter and knn_filter(radius=...) threshold.  Same
// d^2, same r^2 and same compare as cloud_filter.hip's brute-force pass, so the two routes take the same decision on every pair
// they both test; the grid only leaves out pairs that are too far apart to count.
//
// Fixed-radius self-join (pplie_nbr_grid).  Grid = (tiles of 256 consecutive entries of the SORTED planes) x (batch).  The
// queries are the indexed cloud itself, so a lane reads its point straight from the planes (coalesced; no query permutation, no
// second sort, no SE3 row) and a workgroup's 256 points already share a few neighbouring cells.  The lane keeps one int32 count.
//
// Box.  The radius is given, so the cells a lane has to visit are known before the first pair is tested: per axis
// cell(rel - rho) .. cell(rel + rho), rel = p - min, rho = sqrt(r^2) (1 + 2^-10) + h 2^-10 (knn_grid.hip's safety margin: a cell
// is off by a few eps of the extent <= 128 h, a difference of coordinates by one rounding).  cell() is monotone and is the
// arithmetic the points were binned with, so no point with d^2 <= r^2 lies outside the range; the margin only ever adds pairs,
// the compare d^2 <= r^2 alone decides one.  The workgroup box is the union over its lanes (DPP in the wave, LDS across the four
// waves), clamped by cell() itself.  It is formed once: no certification, no list, no rescan.
//
// Stream.  The box's by x bz runs of the sorted planes with their prefix sums sit in LDS, kGridRuns at a time, and the
// concatenated runs go through two 1024-point LDS buffers of THREE planes (the count needs no index plane), the next tile in
// flight in registers (knn_grid_box.h, shared with the k-NN query).  Inner loop: cloud_filter.hip's K = 0 loop -- broadcast 16-byte
// LDS reads, four neighbours per trip, dx^2 + dy^2 + dz^2 in the same operation order, count += (d^2 <= r^2).  The point itself is
// counted through d = 0; the +inf padding behind the stream never counts.
//
// Early stop.  After a tile the workgroup leaves when every live lane has count > stop.  The caller's threshold is
// count - 1 >= nbr with stop = nbr, so a count frozen above nbr gives the same mask; a dense cluster (thousands of points in one
// cell) then costs a tile or two instead of its whole run.  stop = INT_MAX: exact counts.  The result is scattered through the
// index's original indices, four bytes per point, into [B, 1, N]: pplie_nbr_finish's layout with S = 1.
#include "knn_grid_box.h"

namespace pplie {

template <class T> struct NbrGridArgs {
  const T* planes; const int* oidx; const int* starts;   // [3, B N], [B N], [cells + 1]
  const double* hdr; const int* cbase;                   // [B, 8], [B]
  int* pcount;                                           // [B, 1, N], original point order
  int64_t N, Ntot;
  T r2;
  int stop;
};

template <class T>
__global__ void __launch_bounds__(kKnnBlock)
nbr_grid_kernel(NbrGridArgs<T> a) {
  typedef typename KnnV4<T>::type V4;
  __shared__ __attribute__((aligned(32))) T lds[2][3 * kKnnTile];
  __shared__ int rbeg[kGridRuns], rpre[kGridRuns];
  __shared__ float red[kKnnBlock / 64][6];
  __shared__ int sbox[6];
  __shared__ double wsum[kKnnBlock / 64];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.y, slot = (int64_t)blockIdx.x * kKnnBlock + tid;
  const bool act = slot < a.N;
  const int64_t self = b * a.N + (act ? slot : 0);       // sorted position: the keys ascend with the batch element

  const GridHeader<T> G(a.hdr + b * kGridHdr);
  const int cb = a.cbase[b];
  const T* gx = a.planes;
  const T* gy = gx + a.Ntot;
  const T* gz = gy + a.Ntot;
  const T px = gx[self], py = gy[self], pz = gz[self];

  // ---- the box, once: the cells within rho of the lane's point, then the union over the workgroup
  const T rho = pp_sqrt(a.r2) * (T(1) + T(1) / T(1024)) + G.h / T(1024);
  const T rel[3] = {px - G.mn[0], py - G.mn[1], pz - G.mn[2]};
  int lo[3], hi[3], blo[3], bhi[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    lo[c] = grid_cell<T>(rel[c] - rho, G.h, G.g[c]);
    hi[c] = grid_cell<T>(rel[c] + rho, G.h, G.g[c]);
  }
  grid_box_union(act, lo, hi, G.g, true, red, sbox, blo, bhi);

  int cnt = 0;
  bool more = true;                                      // (uniform over the workgroup)
  const int by = bhi[1] - blo[1] + 1, nruns = by * (bhi[2] - blo[2] + 1);
  for (int r0 = 0; more && r0 < nruns; r0 += kGridRuns) {
    const int nr = nruns - r0 < kGridRuns ? nruns - r0 : kGridRuns;
    const int total = grid_run_table(a.starts, cb, G.g, blo, bhi, by, r0, nr, rbeg, rpre, wsum);
    const int ntiles = (total + kKnnTile - 1) / kKnnTile;
    GridFetch<T, false> f;
    if (ntiles > 0) {
      grid_fetch<T, false>(0, total, nr, rbeg, rpre, gx, gy, gz, nullptr, f);
      grid_commit<T, false>(f, lds[0], nullptr);
    }
    __syncthreads();
    for (int t = 0; more && t < ntiles; ++t) {
      const int cur = t & 1;
      const bool next = t + 1 < ntiles;
      if (next) grid_fetch<T, false>(t + 1, total, nr, rbeg, rpre, gx, gy, gz, nullptr, f);      // in flight during this tile

      const T* sx = lds[cur];
      const T* sy = sx + kKnnTile;
      const T* sz = sy + kKnnTile;
      const int left = total - t * kKnnTile, n4 = ((left < kKnnTile ? left : kKnnTile) + 3) & ~3;   // (the padding is x = +inf)
      V4 nX = *reinterpret_cast<const V4*>(sx), nY = *reinterpret_cast<const V4*>(sy), nZ = *reinterpret_cast<const V4*>(sz);
#pragma unroll 2
      for (int j = 0; j < n4; j += 4) {
        const V4 X = nX, Y = nY, Z = nZ;
        const int jn = j + 4 < n4 ? j + 4 : j;
        nX = *reinterpret_cast<const V4*>(sx + jn);
        nY = *reinterpret_cast<const V4*>(sy + jn);
        nZ = *reinterpret_cast<const V4*>(sz + jn);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const T dx = X[q] - px, dy = Y[q] - py, dz = Z[q] - pz;
          const T dd = knn_fma(dz, dz, knn_fma(dy, dy, dx * dx));
          cnt += dd <= a.r2 ? 1 : 0;
        }
      }

      if (next) grid_commit<T, false>(f, lds[cur ^ 1], nullptr);
      // the other buffer is complete and every lane is done reading this one; and: is any live lane still at or below `stop`?
      more = __syncthreads_or(act && cnt <= a.stop) != 0;
    }
    __syncthreads();                                     // every lane is done with the run table
  }

  if (act) a.pcount[b * a.N + a.oidx[self]] = cnt;
}

template <class T>
int launch_nbr_grid(const void* planes, const void* oidx, const void* starts, const void* hdr, const void* cbase, void* pcount,
                    double r2, int stop, int64_t B, int64_t N, void* stream) {
  if (B < 0 || N < 0 || !(r2 >= 0) || !((double)(T)r2 < __builtin_huge_val())) return PPLIE_EBADARG;
  if (B > 65535 || N >= (int64_t(1) << 31) || B * N > (int64_t(1) << 30)) return PPLIE_EUNSUPPORTED;
  if (B == 0 || N == 0) return PPLIE_OK;
  if (!planes || !oidx || !starts || !hdr || !cbase || !pcount) return PPLIE_EBADARG;
  NbrGridArgs<T> a;
  a.planes = static_cast<const T*>(planes); a.oidx = static_cast<const int*>(oidx); a.starts = static_cast<const int*>(starts);
  a.hdr = static_cast<const double*>(hdr); a.cbase = static_cast<const int*>(cbase); a.pcount = static_cast<int*>(pcount);
  a.N = N; a.Ntot = B * N; a.r2 = (T)r2; a.stop = stop;
  hipLaunchKernelGGL((nbr_grid_kernel<T>), dim3((unsigned)((N + kKnnBlock - 1) / kKnnBlock), (unsigned)B), dim3(kKnnBlock), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return knn_status();
}

}  // namespace pplie

#define PPLIE_NBR_GRID_ENTRIES(SFX, T)                                                                                                 \
  extern "C" int pplie_nbr_grid_##SFX(const void* planes, const void* oidx, const void* starts, const void* hdr, const void* cbase,   \
                                      void* pcount, double r2, int stop, int64_t B, int64_t N, void* stream) {                         \
    return pplie::launch_nbr_grid<T>(planes, oidx, starts, hdr, cbase, pcount, r2, stop, B, N, stream);                                \
  }
PPLIE_NBR_GRID_ENTRIES(f32, float)
PPLIE_NBR_GRID_ENTRIES(f64, double)

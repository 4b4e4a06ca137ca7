// pplie-build: no-packed-fp32
// pplie-build: precise
// knn_grid.hip -- exact k nearest neighbours of 3-D points through a uniform grid over the neighbour cloud, built once and queried
// many times (pp.knn_index; the unmoving target of an ICP loop).  Same d^2, same tie rule and same partial-list output as knn.hip's
// brute-force pass, so the two routes agree bit for bit; what changes is how many pairs are tested.
//
// Build.  (1) pplie_knn_grid_bbox: column minima, maxima and a non-finite flag per batch element, as seven minima (min p, min -p,
// min -bad): inside the wave by DPP, across the four waves through LDS, <= 256 workgroup partials folded by a second small launch
// -- min is exact and order-free, no float atomics.  That launch also chooses the cell size h (one per batch element) for a mean
// of `occ` points per cell of the bounding box, h >= extent / 127.5 so that no axis has more than 128 cells, and leaves the header
// {min (3), h, gx, gy, gz, bad} in fp64 on the device.  g = cell(max) + 1 with the points' own cell arithmetic, so the clamp
// min(., g - 1) never moves a point.  (2) pplie_knn_grid_keys: cell(p) = min(trunc((p - min) / h), g - 1) per axis, key =
// base_b + (z gy + y) gx + x, x fastest: every x-row of cells is one contiguous run of the sorted cloud.  (3) after torch.sort
// (stable; plumbing) pplie_knn_grid_tables gathers the sorted cloud into three planes x[] y[] z[], writes the int32 original
// indices, and one lane per cell finds the cell's start by a lower bound over the sorted keys (balanced, and an empty cell gets
// the start of the next occupied one without a serial gap fill).
//
// Query (pplie_knn_grid).  Grid = (tiles of 256 query points) x (batch); one lane owns one query point (moved by the batch
// element's SE3 row on load) and its sorted best-K list in registers, K in {1, 2, 4, 8, 16} >= k.  The workgroup reduces its lanes'
// cells to one box (DPP + LDS), clamps it to the grid -- a query may lie anywhere -- and grows it by a cell on each side.  The box
// is by x bz runs of the sorted planes; their starts and the prefix sums of their lengths sit in LDS in chunks of 256 runs, and
// the concatenated runs stream through knn.hip's two 1024-point LDS buffers: a lane finds the run of each of its four stream
// positions by a binary search of the prefix sums and loads x, y, z and the original index (lane-contiguous inside a run, +inf
// padding behind the end), the next tile in flight in registers while the current one is computed on.  The inner loop is
// knn.hip's: broadcast 16-byte LDS reads, four neighbours per trip, dx^2 + dy^2 + dz^2 in the same operation order.  Candidates
// do not arrive in ascending index, so the list is ordered by (d^2, original index) (knn_insert_lex): the stable-sort order.
//
// Certification.  After a pass a lane is closed when its list is full and d[K-1] <= bound^2, bound = the smallest distance from
// its point to a box face with unvisited cells behind it (+inf for faces on the grid boundary), shrunk by 2^-10 relative and by
// h 2^-10: a point's cell is off by a few eps of the extent <= 128 h, and a difference of coordinates by one rounding.  If a lane
// stays open, the open lanes ask for the cells that cover the sphere of radius sqrt(d[K-1]) plus one cell (or, with a list not yet
// full, for the box grown by half its size on each side), the workgroup takes the union, at least the old box grown by one cell
// (so the loop ends after at most 128 passes, at the whole grid), the open lanes reset their lists and rescan; closed lanes take
// no insertions.  Correctness does not depend on how the queries are ordered: a scattered tile degenerates to brute force.
// (The cell arithmetic, the box union, the run table and the stream loaders live in knn_grid_box.h, shared with nbr_grid.hip.)
#include "knn_grid_box.h"

namespace pplie {

constexpr int kGridParts = 256;      // workgroups per batch element of the bounding-box launch
constexpr int kGridRed = 7;          // min p (3), min -p (3), min -bad

// the kGridRed minima over the workgroup's lanes, in red[0][.] after the call (every lane calls it; barriers inside)
template <class T> __device__ __forceinline__ void grid_block_min(const T* m, T (*red)[kGridRed]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < kGridRed; ++c) {
    const T t = wave_min63<T>(m[c]);
    if (lane == 63) red[wave][c] = t;
  }
  __syncthreads();
  if (threadIdx.x < kGridRed) {
    const int c = threadIdx.x;
    red[0][c] = knn_min(knn_min(red[0][c], red[1][c]), knn_min(red[2][c], red[3][c]));
  }
  __syncthreads();
}

template <class T>
__global__ void __launch_bounds__(kGridBlock)
grid_bbox_kernel(const T* __restrict__ cloud, int64_t N, T* __restrict__ part) {
  __shared__ T red[kGridBlock / 64][kGridRed];
  T m[kGridRed];
#pragma unroll
  for (int c = 0; c < kGridRed; ++c) m[c] = knn_inf<T>();
  const T* cl = cloud + (int64_t)blockIdx.y * N * 3;
  for (int64_t i = (int64_t)blockIdx.x * kGridBlock + threadIdx.x; i < N; i += (int64_t)gridDim.x * kGridBlock) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const T v = cl[i * 3 + c];
      m[c] = knn_min(m[c], v);
      m[3 + c] = knn_min(m[3 + c], -v);
      if (!(__builtin_fabs((double)v) < (double)knn_inf<T>())) m[6] = T(-1);
    }
  }
  grid_block_min<T>(m, red);
  if (threadIdx.x < kGridRed) part[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kGridRed + threadIdx.x] = red[0][threadIdx.x];
}

template <class T>
__global__ void __launch_bounds__(kGridBlock)
grid_header_kernel(const T* __restrict__ part, int P, int64_t N, double occ, double* __restrict__ hdr) {
  __shared__ T red[kGridBlock / 64][kGridRed];
  T m[kGridRed];
#pragma unroll
  for (int c = 0; c < kGridRed; ++c)
    m[c] = (int)threadIdx.x < P ? part[((int64_t)blockIdx.x * P + threadIdx.x) * kGridRed + c] : knn_inf<T>();     // P <= the workgroup size
  grid_block_min<T>(m, red);
  if (threadIdx.x != 0) return;
  T mn[3], ext[3];
  double vol = 1.0, longest = 0.0;
  int nd = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    mn[c] = red[0][c];
    ext[c] = -red[0][3 + c] - mn[c];
    if (ext[c] > T(0)) {                                 // a degenerate axis takes no part in the cell volume
      vol *= (double)ext[c];
      longest = longest > (double)ext[c] ? longest : (double)ext[c];
      ++nd;
    }
  }
  const double per = vol * occ / (double)N;              // volume (area, length) of a cell that holds occ points on average
  double hd = nd == 3 ? ::cbrt(per) : nd == 2 ? ::sqrt(per) : nd == 1 ? per : 1.0;
  hd = hd > longest / 127.5 ? hd : longest / 127.5;      // trunc(extent / h) <= 127 with room for the roundings
  T h = (T)hd;
  if (!(h > T(0)) || !(h < knn_inf<T>())) h = T(1);      // (an extent that underflows, or a cloud that is flagged anyway)
  double* H = hdr + (int64_t)blockIdx.x * kGridHdr;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    H[c] = (double)mn[c];
    H[4 + c] = (double)(grid_cell<T>(ext[c], h, kGridMaxAxis) + 1);
  }
  H[3] = (double)h;
  H[7] = red[0][6] < T(0) ? 1.0 : 0.0;
}

// cbase: first cell of every batch element in the cell table, or NULL: 2^21 = 128^3 cells apart (a key to sort by, no table)
template <class T>
__global__ void __launch_bounds__(kGridBlock)
grid_keys_kernel(const T* __restrict__ cloud, int64_t N, const double* __restrict__ hdr, const int* __restrict__ cbase,
                 int* __restrict__ keys) {
  const int64_t b = blockIdx.y, i = (int64_t)blockIdx.x * kGridBlock + threadIdx.x;
  if (i >= N) return;
  const GridHeader<T> G(hdr + b * kGridHdr);
  const T* p = cloud + (b * N + i) * 3;
  int c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) c[a] = grid_cell<T>(p[a] - G.mn[a], G.h, G.g[a]);
  keys[b * N + i] = (cbase ? cbase[b] : (int)(b << 21)) + (c[2] * G.g[1] + c[1]) * G.g[0] + c[0];
}

template <class T>
__global__ void __launch_bounds__(kGridBlock)
grid_gather_kernel(const T* __restrict__ cloud, const int64_t* __restrict__ perm, int64_t Ntot, int64_t N, T* __restrict__ planes,
                   int* __restrict__ oidx) {
  const int64_t i = (int64_t)blockIdx.x * kGridBlock + threadIdx.x;
  if (i >= Ntot) return;
  const int64_t j = perm[i];                             // the keys ascend with the batch element: j is in i's element
  planes[i] = cloud[j * 3];
  planes[Ntot + i] = cloud[j * 3 + 1];
  planes[2 * Ntot + i] = cloud[j * 3 + 2];
  oidx[i] = (int)(j % N);
}

// starts[c] = the first sorted position whose key is >= c, for c in [0, ncells]: an empty cell starts where the next one does
__global__ void __launch_bounds__(kGridBlock)
grid_starts_kernel(const int* __restrict__ keys, int64_t Ntot, int ncells, int* __restrict__ starts) {
  const int64_t c = (int64_t)blockIdx.x * kGridBlock + threadIdx.x;
  if (c > ncells) return;
  int64_t lo = 0, hi = Ntot;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  starts[c] = (int)lo;
}

template <class T> struct KnnGridArgs {
  const T* ref; const T* tf; const int64_t* qperm;       // tf: SE3 rows [B, 7] or NULL; qperm: the order to take the queries in, or NULL
  const T* planes; const int* oidx; const int* starts;   // [3, Ntot], [Ntot], [cells + 1]
  const double* hdr; const int* cbase;                   // [Bi, 8], [Bi]
  T* pd2; int* pidx;                                     // [B, 1, N1, k]
  int64_t N1, Ntot, ref_bstride, perm_bstride;           // strides in points, 0 = shared by the batch
  int k, idx_bstride;                                    // 0: one index for the whole batch, 1: one per batch element
};

template <class T, int K>
__global__ void __launch_bounds__(kKnnBlock)
knn_grid_kernel(KnnGridArgs<T> a) {
  typedef typename KnnV4<T>::type V4;
  __shared__ __attribute__((aligned(32))) T lds[2][3 * kKnnTile];
  __shared__ __attribute__((aligned(16))) int lid[2][kKnnTile];
  __shared__ int rbeg[kGridRuns], rpre[kGridRuns];
  __shared__ float red[kKnnBlock / 64][6];
  __shared__ int sbox[6];
  __shared__ double wsum[kKnnBlock / 64];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.y, slot = (int64_t)blockIdx.x * kKnnBlock + tid;
  const bool act = slot < a.N1;
  const int64_t row = !act ? 0 : a.qperm ? a.qperm[b * a.perm_bstride + slot] - b * a.perm_bstride : slot;

  const GridHeader<T> G(a.hdr + b * a.idx_bstride * kGridHdr);
  const int cb = a.cbase[b * a.idx_bstride];
  const T* gx = a.planes;
  const T* gy = gx + a.Ntot;
  const T* gz = gy + a.Ntot;

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
  const T rel[3] = {px - G.mn[0], py - G.mn[1], pz - G.mn[2]};
  T d[K];
  int id[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    d[i] = knn_inf<T>();
    id[i] = -1;
  }

  bool open = act, first = true;
  int lo[3], hi[3], blo[3] = {0, 0, 0}, bhi[3] = {0, 0, 0};          // the lane's wish (cells, may leave the grid by one); the box
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int cell = grid_cell<T>(rel[c], G.h, G.g[c]);
    lo[c] = cell - 1;
    hi[c] = cell + 1;
  }
  const T shrink = T(1) - T(1) / T(1024), slack = G.h / T(1024);

  for (;;) {
    // ---- the box: union of the open lanes' wishes and of the previous box grown by a cell, clamped to the grid
    grid_box_union(open, lo, hi, G.g, first, red, sbox, blo, bhi);
    first = false;
    const bool whole = blo[0] == 0 && blo[1] == 0 && blo[2] == 0 && bhi[0] == G.g[0] - 1 && bhi[1] == G.g[1] - 1 && bhi[2] == G.g[2] - 1;

    // ---- the box's runs (one per (y, z): cells blo[0] .. bhi[0] are contiguous in the sorted planes), kGridRuns at a time
    const int by = bhi[1] - blo[1] + 1, nruns = by * (bhi[2] - blo[2] + 1);
    for (int r0 = 0; r0 < nruns; r0 += kGridRuns) {
      const int nr = nruns - r0 < kGridRuns ? nruns - r0 : kGridRuns;
      const int total = grid_run_table(a.starts, cb, G.g, blo, bhi, by, r0, nr, rbeg, rpre, wsum);
      const int ntiles = (total + kKnnTile - 1) / kKnnTile;
      GridFetch<T, true> f;
      if (ntiles > 0) {
        grid_fetch<T, true>(0, total, nr, rbeg, rpre, gx, gy, gz, a.oidx, f);
        grid_commit<T, true>(f, lds[0], lid[0]);
      }
      __syncthreads();
      for (int t = 0; t < ntiles; ++t) {
        const int cur = t & 1;
        const bool next = t + 1 < ntiles;
        if (next) grid_fetch<T, true>(t + 1, total, nr, rbeg, rpre, gx, gy, gz, a.oidx, f);                       // in flight while this tile is computed on

        const T* sx = lds[cur];
        const T* sy = sx + kKnnTile;
        const T* sz = sy + kKnnTile;
        const int* si = lid[cur];
        const int left = total - t * kKnnTile, cnt = ((left < kKnnTile ? left : kKnnTile) + 3) & ~3;
        V4 nX = *reinterpret_cast<const V4*>(sx), nY = *reinterpret_cast<const V4*>(sy), nZ = *reinterpret_cast<const V4*>(sz);
#pragma unroll 2
        for (int j = 0; j < cnt; j += 4) {
          const V4 X = nX, Y = nY, Z = nZ;
          const int jn = j + 4 < cnt ? j + 4 : j;
          nX = *reinterpret_cast<const V4*>(sx + jn);
          nY = *reinterpret_cast<const V4*>(sy + jn);
          nZ = *reinterpret_cast<const V4*>(sz + jn);
          T dd[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const T dx = X[q] - px, dy = Y[q] - py, dz = Z[q] - pz;
            dd[q] = knn_fma(dz, dz, knn_fma(dy, dy, dx * dx));
          }
          if (open && knn_min(knn_min(dd[0], dd[1]), knn_min(dd[2], dd[3])) <= d[K - 1]) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const int ci = si[j + q];
              if (knn_before<T>(dd[q], ci, d[K - 1], id[K - 1])) knn_insert_lex<T, K>(d, id, dd[q], ci);
            }
          }
        }

        if (next) grid_commit<T, true>(f, lds[cur ^ 1], lid[cur ^ 1]);
        __syncthreads();                                 // the other buffer is complete; every lane is done reading this one
      }
      __syncthreads();                                   // ... and with the run table
    }

    // ---- certification
    if (open) {
      T face = knn_inf<T>();
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (blo[c] > 0) face = knn_min(face, rel[c] - T(blo[c]) * G.h);
        if (bhi[c] < G.g[c] - 1) face = knn_min(face, T(bhi[c] + 1) * G.h - rel[c]);
      }
      const T bound = face * shrink - slack;
      const bool full = id[K - 1] >= 0;
      if (full && bound > T(0) && d[K - 1] <= bound * bound) {
        open = false;
      } else if (!whole) {
        if (full) {                                      // the cells of the sphere that must be searched, and one more
          const T r = pp_sqrt(d[K - 1]) * (T(1) + T(1) / T(1024)) + slack;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            lo[c] = grid_cell<T>(rel[c] - r, G.h, G.g[c]) - 1;
            hi[c] = grid_cell<T>(rel[c] + r, G.h, G.g[c]) + 1;
          }
        } else {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int half = (bhi[c] - blo[c] + 2) / 2;
            lo[c] = blo[c] - half < -1 ? -1 : blo[c] - half;
            hi[c] = bhi[c] + half > kGridMaxAxis ? kGridMaxAxis : bhi[c] + half;
          }
        }
#pragma unroll
        for (int i = 0; i < K; ++i) {
          d[i] = knn_inf<T>();
          id[i] = -1;
        }
      }
    }
    if (whole) break;                                    // every point of the element has been visited
    if (!__syncthreads_or(open)) break;
  }

  if (!act) return;
  const int64_t o = (b * a.N1 + row) * a.k;
#pragma unroll
  for (int j = 0; j < K; ++j)
    if (j < a.k) {
      a.pd2[o + j] = d[j];
      a.pidx[o + j] = id[j];
    }
}

// ---- launchers
inline bool grid_shape_ok(int64_t B, int64_t N) { return B <= 65535 && N < (int64_t(1) << 31) && B * N <= (int64_t(1) << 30); }

template <class T>
int launch_grid_bbox(const void* cloud, int64_t B, int64_t N, double occ, void* part, void* hdr, void* stream) {
  if (B < 0 || N < 0 || !(occ > 0)) return PPLIE_EBADARG;
  if (!grid_shape_ok(B, N)) return PPLIE_EUNSUPPORTED;
  if (B == 0 || N == 0) return PPLIE_OK;
  if (!cloud || !part || !hdr) return PPLIE_EBADARG;
  const int64_t nwg = (N + kGridBlock - 1) / kGridBlock;
  const int P = (int)(nwg < kGridParts ? nwg : kGridParts);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL((grid_bbox_kernel<T>), dim3((unsigned)P, (unsigned)B), dim3(kGridBlock), 0, st, static_cast<const T*>(cloud), N,
                     static_cast<T*>(part));
  hipLaunchKernelGGL((grid_header_kernel<T>), dim3((unsigned)B), dim3(kGridBlock), 0, st, static_cast<const T*>(part), P, N, occ,
                     static_cast<double*>(hdr));
  return knn_status();
}

template <class T>
int launch_grid_keys(const void* cloud, int64_t B, int64_t N, const void* hdr, const void* cbase, void* keys, void* stream) {
  if (B < 0 || N < 0) return PPLIE_EBADARG;
  if (!grid_shape_ok(B, N) || (!cbase && B > 1023)) return PPLIE_EUNSUPPORTED;
  if (B == 0 || N == 0) return PPLIE_OK;
  if (!cloud || !hdr || !keys) return PPLIE_EBADARG;
  hipLaunchKernelGGL((grid_keys_kernel<T>), dim3((unsigned)((N + kGridBlock - 1) / kGridBlock), (unsigned)B), dim3(kGridBlock), 0,
                     reinterpret_cast<hipStream_t>(stream), static_cast<const T*>(cloud), N, static_cast<const double*>(hdr),
                     static_cast<const int*>(cbase), static_cast<int*>(keys));
  return knn_status();
}

template <class T>
int launch_grid_tables(const void* cloud, const void* keys, const void* perm, int64_t B, int64_t N, int64_t ncells, void* planes,
                       void* oidx, void* starts, void* stream) {
  if (B < 0 || N < 0 || ncells < 0) return PPLIE_EBADARG;
  if (!grid_shape_ok(B, N) || ncells > (int64_t(1) << 24)) return PPLIE_EUNSUPPORTED;
  if (B == 0 || N == 0) return PPLIE_OK;
  if (!cloud || !keys || !perm || !planes || !oidx || !starts) return PPLIE_EBADARG;
  const int64_t Ntot = B * N;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL((grid_gather_kernel<T>), dim3((unsigned)((Ntot + kGridBlock - 1) / kGridBlock)), dim3(kGridBlock), 0, st,
                     static_cast<const T*>(cloud), static_cast<const int64_t*>(perm), Ntot, N, static_cast<T*>(planes),
                     static_cast<int*>(oidx));
  hipLaunchKernelGGL(grid_starts_kernel, dim3((unsigned)((ncells + 1 + kGridBlock - 1) / kGridBlock)), dim3(kGridBlock), 0, st,
                     static_cast<const int*>(keys), Ntot, (int)ncells, static_cast<int*>(starts));
  return knn_status();
}

template <class T>
int launch_knn_grid(const void* ref, const void* tf, const void* qperm, const void* planes, const void* oidx, const void* starts,
                    const void* hdr, const void* cbase, void* pd2, void* pidx, int64_t B, int64_t N1, int64_t Ntot, int k,
                    int64_t ref_bstride, int64_t perm_bstride, int idx_bstride, void* stream) {
  if (B < 0 || N1 < 0 || Ntot < 1 || k < 1 || ref_bstride < 0 || perm_bstride < 0 || idx_bstride < 0 || idx_bstride > 1)
    return PPLIE_EBADARG;
  if (k > kKnnMaxK || N1 >= (int64_t(1) << 31) || Ntot > (int64_t(1) << 30) || B > 65535) return PPLIE_EUNSUPPORTED;
  if (B == 0 || N1 == 0) return PPLIE_OK;
  if (!ref || !planes || !oidx || !starts || !hdr || !cbase || !pd2 || !pidx) return PPLIE_EBADARG;
  KnnGridArgs<T> a;
  a.ref = static_cast<const T*>(ref); a.tf = static_cast<const T*>(tf); a.qperm = static_cast<const int64_t*>(qperm);
  a.planes = static_cast<const T*>(planes); a.oidx = static_cast<const int*>(oidx); a.starts = static_cast<const int*>(starts);
  a.hdr = static_cast<const double*>(hdr); a.cbase = static_cast<const int*>(cbase); a.pd2 = static_cast<T*>(pd2);
  a.pidx = static_cast<int*>(pidx); a.N1 = N1; a.Ntot = Ntot; a.ref_bstride = ref_bstride; a.perm_bstride = perm_bstride;
  a.k = k; a.idx_bstride = idx_bstride;
  const dim3 grid((unsigned)((N1 + kKnnBlock - 1) / kKnnBlock), (unsigned)B), block(kKnnBlock);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  switch (knn_width(k)) {
    case 1: hipLaunchKernelGGL((knn_grid_kernel<T, 1>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((knn_grid_kernel<T, 2>), grid, block, 0, st, a); break;
    case 4: hipLaunchKernelGGL((knn_grid_kernel<T, 4>), grid, block, 0, st, a); break;
    case 8: hipLaunchKernelGGL((knn_grid_kernel<T, 8>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((knn_grid_kernel<T, 16>), grid, block, 0, st, a); break;
  }
  return knn_status();
}

}  // namespace pplie

#define PPLIE_KNN_GRID_ENTRIES(SFX, T)                                                                                                  \
  extern "C" int pplie_knn_grid_bbox_##SFX(const void* cloud, int64_t B, int64_t N, double occ, void* part, void* hdr, void* stream) { \
    return pplie::launch_grid_bbox<T>(cloud, B, N, occ, part, hdr, stream);                                                             \
  }                                                                                                                                     \
  extern "C" int pplie_knn_grid_keys_##SFX(const void* cloud, int64_t B, int64_t N, const void* hdr, const void* cbase, void* keys,    \
                                           void* stream) {                                                                             \
    return pplie::launch_grid_keys<T>(cloud, B, N, hdr, cbase, keys, stream);                                                           \
  }                                                                                                                                     \
  extern "C" int pplie_knn_grid_tables_##SFX(const void* cloud, const void* keys, const void* perm, int64_t B, int64_t N,              \
                                             int64_t ncells, void* planes, void* oidx, void* starts, void* stream) {                   \
    return pplie::launch_grid_tables<T>(cloud, keys, perm, B, N, ncells, planes, oidx, starts, stream);                                 \
  }                                                                                                                                     \
  extern "C" int pplie_knn_grid_##SFX(const void* ref, const void* T_, const void* qperm, const void* planes, const void* oidx,        \
                                      const void* starts, const void* hdr, const void* cbase, void* pd2, void* pidx, int64_t B,        \
                                      int64_t N1, int64_t Ntot, int k, int64_t ref_bstride, int64_t perm_bstride, int idx_bstride,     \
                                      void* stream) {                                                                                  \
    return pplie::launch_knn_grid<T>(ref, T_, qperm, planes, oidx, starts, hdr, cbase, pd2, pidx, B, N1, Ntot, k, ref_bstride,          \
                                     perm_bstride, idx_bstride, stream);                                                                \
  }
PPLIE_KNN_GRID_ENTRIES(f32, float)
PPLIE_KNN_GRID_ENTRIES(f64, double)

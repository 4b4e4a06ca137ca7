// pplie-build: no-packed-fp32
// pplie-build: precise
// cloud_filter.hip -- the point-cloud filters that come before registration (nbr_filter, knn_filter, voxel_filter) on clouds
// [N, D], 3 <= D <= 8, whose first three columns are coordinates.  (precise: the voxel cell of a point is trunc((p - min) / v) with
// the IEEE subtraction and the correctly rounded division, so that cell assignment is bit-identical to the tensor formulation's;
// no reciprocal multiply anywhere.)
//
// Self-neighbourhood pass (pplie_nbr_partial).  The work split of knn.hip's partial pass with the cloud streamed against itself:
// grid = (tiles of 256 points) x (S splits of the cloud) x (batch), one lane owns one point (coordinates in registers), the split
// comes through LDS in 1024-point tiles as three planes read with broadcast 16-byte LDS reads, the next tile's global loads in
// flight while the current one is computed on (knn_tile.h).  The lane keeps an int32 count of d^2 <= r^2 and a sorted best-K list,
// K in {0, 1, 2, 4, 8, 16}.  K = 0 is nbr_filter's form: 3 subtractions, 1 multiplication, 2 FMAs, a compare and an add per pair,
// no list.  knn_filter(radius=...) gets count and list from one pass over the pairs.  Direct differences, no matrix instructions,
// for knn.hip's reason (cancellation in |a|^2 + |b|^2 - 2 a.b).  The point itself is among its neighbours: d^2 = 0 is counted and
// heads the list (behind an identical point of smaller index).
//
// Finish (pplie_nbr_finish).  One lane per point adds the S partial counts (integers: order-free), merges the S lists in split order
// (ties to the smaller index), writes the keep mask (count - 1 >= nbr, one byte per point) and, with a list, the mean over the
// k + 1 gathered rows of the full-width cloud, accumulated in fp64 and rounded once.
//
// Voxel keys (pplie_voxel_keys).  Column minima in two launches: per-workgroup minima (inside the wave by DPP, across the four waves
// through LDS) go to <= 256 partials, and every workgroup of the key kernel folds those partials again -- min is exact and
// order-free, so no workgroup waits on or counts another.  One lane per point then packs its three cell indices into one int64 key
// of 3 x 21 bits, i0 in the top field: integer order = lexicographic order.  An index that does not fit raises a flag.
//
// Segmented mean (pplie_voxel_heads, pplie_voxel_reduce) over the stably sorted keys (the sort itself is torch.sort: plumbing).  A
// workgroup takes a slab of 256 sorted entries; a lane is a head when its key differs from the one before.  voxel_heads counts the
// heads of every slab (the exclusive prefix over slabs is the rank of a slab's first head).  voxel_reduce gathers the lane's D-wide
// row and runs a segmented inclusive scan of D sums and a count in fp64: inside the wave by shuffles, the segment start read off the
// ballot of head flags, across the four waves through LDS in wave order.  A run that starts and closes inside the slab is written
// as mean = sum / count, rounded once.  A run that crosses a slab boundary leaves carries -- `lead` (what precedes the slab's first
// head), `tail` (from its last head on) -- and voxel_stitch, one 16-lane group per slab, adds tail + lead + lead ... in slab order up
// to the first slab that has a head.  Every loop is bounded by the slab count; no floating-point atomics: two runs give the same bits.
#include "knn_tile.h"

namespace pplie {

constexpr int kCfBlock = 256;
constexpr int kCfMaxD = 8;
constexpr int kCfCnt = 8;            // column of the count in a carry row
constexpr int kCfCols = 16;          // doubles per carry row: D sums at [0, D), the count at [8]
constexpr int kCfMinParts = 256;     // workgroups of the column-minimum launch
constexpr int kCfCellBits = 21;

template <class T> struct NbrPartialArgs {
  const T* pts;                                          // [B, N, 3]
  int* pcount; T* pd2; int* pidx;                        // [B, S, N], [B, S, N, kk], [B, S, N, kk]
  int64_t N;
  T r2;
  int kk, S, vec;
};

template <class T, int K>
__global__ void __launch_bounds__(kKnnBlock)
nbr_partial_kernel(NbrPartialArgs<T> a) {
  typedef typename KnnV4<T>::type V4;
  constexpr int KL = K > 0 ? K : 1;
  __shared__ __attribute__((aligned(32))) T lds[2][3 * kKnnTile];
  const int tid = threadIdx.x, s = blockIdx.y;
  const int64_t b = blockIdx.z, row = (int64_t)blockIdx.x * kKnnBlock + tid;
  const bool act = row < a.N;
  const T* nb = a.pts + b * a.N * 3;

  T px = T(0), py = T(0), pz = T(0);
  if (act) {
    px = nb[row * 3];
    py = nb[row * 3 + 1];
    pz = nb[row * 3 + 2];
  }
  T d[KL];
  int id[KL];
#pragma unroll
  for (int i = 0; i < KL; ++i) {
    d[i] = knn_inf<T>();
    id[i] = -1;
  }
  int cnt = 0;

  const int64_t ntiles = (a.N + kKnnTile - 1) / kKnnTile;
  const int t0 = (int)(s * ntiles / a.S), t1 = (int)((s + 1) * ntiles / a.S);      // S <= ntiles: no split is empty
  auto full = [&](int t) { return a.vec && (int64_t)(t + 1) * kKnnTile <= a.N; };
  auto valid = [&](int t) { const int64_t left = a.N - (int64_t)t * kKnnTile; return left < kKnnTile ? (int)left : kKnnTile; };

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
    const int n4 = (valid(t) + 3) & ~3, base = t * kKnnTile;                        // (the padding is x = +inf: never <= r^2)
    V4 nX = *reinterpret_cast<const V4*>(sx), nY = *reinterpret_cast<const V4*>(sy), nZ = *reinterpret_cast<const V4*>(sz);
#pragma unroll 2
    for (int j = 0; j < n4; j += 4) {
      const V4 X = nX, Y = nY, Z = nZ;
      const int jn = j + 4 < n4 ? j + 4 : j;
      nX = *reinterpret_cast<const V4*>(sx + jn);
      nY = *reinterpret_cast<const V4*>(sy + jn);
      nZ = *reinterpret_cast<const V4*>(sz + jn);
      T dd[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const T dx = X[q] - px, dy = Y[q] - py, dz = Z[q] - pz;
        dd[q] = knn_fma(dz, dz, knn_fma(dy, dy, dx * dx));
        cnt += dd[q] <= a.r2 ? 1 : 0;
      }
      if constexpr (K > 0) {
        if (knn_min(knn_min(dd[0], dd[1]), knn_min(dd[2], dd[3])) < d[K - 1]) {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (dd[q] < d[K - 1]) knn_insert<T, K>(d, id, dd[q], base + j + q);
        }
      }
    }

    if (next) {
      if (nfull) knn_commit<T>(slab, lds[cur ^ 1]);
      else knn_load_slow<T>(nb + (int64_t)(t + 1) * kKnnTile * 3, valid(t + 1), lds[cur ^ 1]);
    }
    __syncthreads();
  }

  if (!act) return;
  const int64_t o = (b * a.S + s) * a.N + row;
  a.pcount[o] = cnt;
  if constexpr (K > 0) {
#pragma unroll
    for (int j = 0; j < K; ++j)
      if (j < a.kk) {
        a.pd2[o * a.kk + j] = d[j];
        a.pidx[o * a.kk + j] = id[j];
      }
  }
}

template <class T> struct NbrFinishArgs {
  const int* pcount; const T* pd2; const int* pidx;      // [B, S, N], [B, S, N, kk] x 2
  const T* cloud;                                        // [B, N, D] (K > 0)
  unsigned char* mask;                                   // [B, N]
  T* out;                                                // [B, N, D] (K > 0)
  int64_t N;
  int D, kk, S, nbr;
};

template <class T, int K>
__global__ void __launch_bounds__(kCfBlock)
nbr_finish_kernel(NbrFinishArgs<T> a) {
  constexpr int KL = K > 0 ? K : 1;
  const int64_t b = blockIdx.y, row = (int64_t)blockIdx.x * kCfBlock + threadIdx.x;
  if (row >= a.N) return;
  int cnt = 0;
  for (int s = 0; s < a.S; ++s) cnt += a.pcount[(b * a.S + s) * a.N + row];
  a.mask[b * a.N + row] = cnt - 1 >= a.nbr ? 1 : 0;
  if constexpr (K > 0) {
    T d[KL];
    int id[KL];
#pragma unroll
    for (int i = 0; i < K; ++i) {
      d[i] = knn_inf<T>();
      id[i] = -1;
    }
    const int64_t o = (b * a.S * a.N + row) * a.kk;
#pragma unroll
    for (int j = 0; j < K; ++j)
      if (j < a.kk) {
        d[j] = a.pd2[o + j];
        id[j] = a.pidx[o + j];
      }
    for (int s = 1; s < a.S; ++s) {                      // split order = ascending index: a tie keeps the entry it already has
      const int64_t os = ((b * a.S + s) * a.N + row) * a.kk;
      for (int j = 0; j < a.kk; ++j) {
        const T c = a.pd2[os + j];
        if (!(c < d[K - 1])) break;
        knn_insert<T, K>(d, id, c, a.pidx[os + j]);
      }
    }
    double acc[kCfMaxD];
#pragma unroll
    for (int c = 0; c < kCfMaxD; ++c) acc[c] = 0.0;
#pragma unroll
    for (int j = 0; j < K; ++j)
      if (j < a.kk) {
        const int64_t q = id[j] < 0 ? 0 : id[j];         // (a row that matched nothing: keep the gather inside the cloud)
        const T* p = a.cloud + (b * a.N + q) * a.D;
#pragma unroll
        for (int c = 0; c < kCfMaxD; ++c)
          if (c < a.D) acc[c] += (double)p[c];
      }
    T* w = a.out + (b * a.N + row) * a.D;
#pragma unroll
    for (int c = 0; c < kCfMaxD; ++c)
      if (c < a.D) w[c] = (T)(acc[c] / (double)a.kk);
  }
}

// ---- voxel keys (wave_min63: knn_tile.h)
// the three column minima over the workgroup's lanes, left in mn[0..2] (every lane calls it; a barrier follows inside)
template <class T> __device__ __forceinline__ void block_min3(const T* m, T (*red)[3], T* mn) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const T t = wave_min63<T>(m[c]);
    if (lane == 63) red[wave][c] = t;
  }
  __syncthreads();
  if (threadIdx.x < 3) mn[threadIdx.x] = knn_min(knn_min(red[0][threadIdx.x], red[1][threadIdx.x]), knn_min(red[2][threadIdx.x], red[3][threadIdx.x]));
  __syncthreads();
}

template <class T>
__global__ void __launch_bounds__(kCfBlock)
voxel_min_kernel(const T* __restrict__ cloud, int64_t N, int D, T* __restrict__ part) {
  __shared__ T red[kCfBlock / 64][3];
  __shared__ T mn[3];
  T m[3] = {knn_inf<T>(), knn_inf<T>(), knn_inf<T>()};
  for (int64_t i = (int64_t)blockIdx.x * kCfBlock + threadIdx.x; i < N; i += (int64_t)gridDim.x * kCfBlock) {
    const T* p = cloud + i * D;
#pragma unroll
    for (int c = 0; c < 3; ++c) m[c] = knn_min(m[c], p[c]);
  }
  block_min3<T>(m, red, mn);
  if (threadIdx.x < 3) part[blockIdx.x * 3 + threadIdx.x] = mn[threadIdx.x];
}

template <class T>
__global__ void __launch_bounds__(kCfBlock)
voxel_keys_kernel(const T* __restrict__ cloud, int64_t N, int D, const T* __restrict__ part, int npart, T v0, T v1, T v2,
                  int64_t* __restrict__ keys, int* __restrict__ flag) {
  __shared__ T red[kCfBlock / 64][3];
  __shared__ T mn[3];
  T m[3] = {knn_inf<T>(), knn_inf<T>(), knn_inf<T>()};
  if ((int)threadIdx.x < npart) {                        // npart <= kCfMinParts = the workgroup size
#pragma unroll
    for (int c = 0; c < 3; ++c) m[c] = part[threadIdx.x * 3 + c];
  }
  block_min3<T>(m, red, mn);
  const int64_t i = (int64_t)blockIdx.x * kCfBlock + threadIdx.x;
  if (i >= N) return;
  const T* p = cloud + i * D;
  const T v[3] = {v0, v1, v2};
  int64_t key = 0;
  bool bad = false;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    T q = (p[c] - mn[c]) / v[c];                         // IEEE subtraction, correctly rounded division: torch's quotient
    if (!(q < T(1 << kCfCellBits))) {                    // (also a NaN)
      bad = true;
      q = T(0);
    }
    key = (key << kCfCellBits) | (int64_t)q;             // q >= 0: p >= min and v > 0; the conversion truncates
  }
  keys[i] = key;
  if (bad) *flag = 1;
}

// ---- segmented mean over the sorted keys
__global__ void __launch_bounds__(kCfBlock)
voxel_heads_kernel(const int64_t* __restrict__ keys, int64_t N, int* __restrict__ heads) {
  __shared__ int wcnt[kCfBlock / 64];
  const int64_t i = (int64_t)blockIdx.x * kCfBlock + threadIdx.x;
  const bool head = i < N && (i == 0 || keys[i] != keys[i - 1]);
  const unsigned long long bal = __ballot(head);
  if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = __popcll(bal);
  __syncthreads();
  if (threadIdx.x == 0) heads[blockIdx.x] = (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
}

template <class T> struct VoxelReduceArgs {
  const int64_t* keys; const int64_t* perm;              // sorted keys [N], the sort's permutation [N]
  const T* cloud;                                        // [N, D]
  const int64_t* base;                                   // [nWG] heads in the slabs before this one
  double* lead; double* tail; int* info;                 // [nWG, 16], [nWG, 16], [nWG, 4] = {has a head, open, last rank, last start}
  T* out; int* start; int* count;                        // [M, D], [M], [M]
  int64_t N;
  int D, nwg;
};

template <class T>
__global__ void __launch_bounds__(kCfBlock)
voxel_reduce_kernel(VoxelReduceArgs<T> a) {
  constexpr int NC = kCfCnt + 1;
  __shared__ double wtot[kCfBlock / 64][NC];
  __shared__ int whead[kCfBlock / 64], wcnt[kCfBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, D = a.D;
  const int64_t g = blockIdx.x, i = g * kCfBlock + tid;
  const bool valid = i < a.N;
  bool head = false, end = false;
  double v[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) v[c] = 0.0;
  if (valid) {
    const int64_t key = a.keys[i];
    head = i == 0 || a.keys[i - 1] != key;
    end = i == a.N - 1 || a.keys[i + 1] != key;
    const T* p = a.cloud + a.perm[i] * D;
#pragma unroll
    for (int c = 0; c < kCfMaxD; ++c)
      if (c < D) v[c] = (double)p[c];
    v[kCfCnt] = 1.0;
  }

  // inside the wave: lane i sums over [max(segstart, i - 2 off + 1), i] after the step `off`
  const unsigned long long bal = __ballot(head), le = bal & (~0ull >> (63 - lane));
  const int segstart = le ? 63 - __clzll((long long)le) : 0;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < D || c == kCfCnt) {
        const double u = __shfl_up(v[c], off, 64);
        if (lane - off >= segstart) v[c] += u;
      }
  }
  if (lane == 63) {
#pragma unroll
    for (int c = 0; c < NC; ++c) wtot[wave][c] = v[c];
    whead[wave] = bal != 0;
    wcnt[wave] = __popcll(bal);
  }
  __syncthreads();
  // across the waves, in wave order: what the earlier waves leave open
  double carry[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) carry[c] = 0.0;
  int nh = __popcll(le);                                 // heads of the slab up to and including this lane
  bool hs = le != 0;                                     // ... is there one?
  for (int u = 0; u < wave; ++u) {
    const bool h = whead[u] != 0;
#pragma unroll
    for (int c = 0; c < NC; ++c) carry[c] = h ? wtot[u][c] : carry[c] + wtot[u][c];
    nh += wcnt[u];
    hs = hs || h;
  }
  if (le == 0) {                                         // no head in this wave up to the lane: its run began in an earlier wave
#pragma unroll
    for (int c = 0; c < NC; ++c) v[c] = carry[c] + v[c];
  }

  if (!valid) return;
  const int64_t lastvalid = (a.N < (g + 1) * kCfBlock ? a.N : (g + 1) * kCfBlock) - 1;
  const bool last = i == lastvalid;
  const int64_t rank = a.base[g] + nh - 1;
  const int64_t cnt = (int64_t)v[kCfCnt];
  if (hs && end) {                                       // a run that starts and closes inside the slab
    T* w = a.out + rank * D;
#pragma unroll
    for (int c = 0; c < kCfMaxD; ++c)
      if (c < D) w[c] = (T)(v[c] / v[kCfCnt]);
    a.start[rank] = (int)(i - (cnt - 1));
    a.count[rank] = (int)cnt;
  }
  double* ld = a.lead + g * kCfCols;
  if (!hs && (end || last)) {                            // what precedes the slab's first head (the whole slab if it has none)
#pragma unroll
    for (int c = 0; c < NC; ++c) ld[c] = v[c];
  }
  if (tid == 0 && head) {
#pragma unroll
    for (int c = 0; c < NC; ++c) ld[c] = 0.0;
  }
  if (last) {
    if (hs) {
      double* tl = a.tail + g * kCfCols;
#pragma unroll
      for (int c = 0; c < NC; ++c) tl[c] = v[c];
    }
    int* in = a.info + g * 4;
    in[0] = hs;
    in[1] = hs && !end;
    in[2] = (int)rank;
    in[3] = (int)(i - (cnt - 1));
  }
}

// the runs that cross a slab boundary: 16 lanes per slab (lane c carries column c), carries added in slab order
template <class T>
__global__ void __launch_bounds__(kCfBlock)
voxel_stitch_kernel(VoxelReduceArgs<T> a) {
  const int64_t t = (int64_t)blockIdx.x * kCfBlock + threadIdx.x, g = t / kCfCols;
  const int c = (int)(t % kCfCols), lane = threadIdx.x & 63;
  const bool used = c < a.D || c == kCfCnt;
  const bool open = g < a.nwg && a.info[g * 4 + 1] != 0;
  double sum = 0.0;
  if (open && used) {
    sum = a.tail[g * kCfCols + c];
    for (int64_t h = g + 1; h < a.nwg; ++h) {
      sum += a.lead[h * kCfCols + c];
      if (a.info[h * 4] != 0) break;                     // the run closes in the first slab that has a head
    }
  }
  const double cnt = __shfl(sum, (lane & ~(kCfCols - 1)) | kCfCnt, 64);
  if (open && used) {
    const int64_t rank = a.info[g * 4 + 2];
    if (c < a.D) {
      a.out[rank * a.D + c] = (T)(sum / cnt);
    } else {
      a.start[rank] = a.info[g * 4 + 3];
      a.count[rank] = (int)cnt;
    }
  }
}

// ---- launchers
inline bool cf_shape_ok(int64_t N, int D) { return N < (int64_t(1) << 31) && D >= 3 && D <= kCfMaxD; }

template <class T>
int launch_nbr_partial(const void* pts, void* pcount, void* pd2, void* pidx, int64_t B, int64_t N, double r2, int kk, int S,
                       void* stream) {
  if (B < 0 || N < 0 || kk < 0 || S < 1 || !(r2 == r2)) return PPLIE_EBADARG;
  if (kk > kKnnMaxK || N >= (int64_t(1) << 31) || B > 65535) return PPLIE_EUNSUPPORTED;
  if (kk > N) return PPLIE_EBADARG;
  if (B == 0 || N == 0) return PPLIE_OK;
  const int64_t ntiles = (N + kKnnTile - 1) / kKnnTile;
  if (S > ntiles || S > 65535) return PPLIE_EBADARG;
  if (!pts || !pcount || (kk > 0 && (!pd2 || !pidx))) return PPLIE_EBADARG;
  NbrPartialArgs<T> a;
  a.pts = static_cast<const T*>(pts); a.pcount = static_cast<int*>(pcount); a.pd2 = static_cast<T*>(pd2);
  a.pidx = static_cast<int*>(pidx); a.N = N; a.r2 = (T)r2; a.kk = kk; a.S = S;
  a.vec = aligned16(pts) && (B == 1 || (N * 3 * (int64_t)sizeof(T)) % 16 == 0);     // every tile slab starts on 16 bytes
  const dim3 grid((unsigned)((N + kKnnBlock - 1) / kKnnBlock), (unsigned)S, (unsigned)B), block(kKnnBlock);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  switch (kk == 0 ? 0 : knn_width(kk)) {
    case 0: hipLaunchKernelGGL((nbr_partial_kernel<T, 0>), grid, block, 0, st, a); break;
    case 1: hipLaunchKernelGGL((nbr_partial_kernel<T, 1>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((nbr_partial_kernel<T, 2>), grid, block, 0, st, a); break;
    case 4: hipLaunchKernelGGL((nbr_partial_kernel<T, 4>), grid, block, 0, st, a); break;
    case 8: hipLaunchKernelGGL((nbr_partial_kernel<T, 8>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((nbr_partial_kernel<T, 16>), grid, block, 0, st, a); break;
  }
  return knn_status();
}

template <class T>
int launch_nbr_finish(const void* pcount, const void* pd2, const void* pidx, const void* cloud, void* mask, void* out, int64_t B,
                      int64_t N, int D, int kk, int S, int nbr, void* stream) {
  if (B < 0 || N < 0 || kk < 0 || S < 1) return PPLIE_EBADARG;
  if (kk > kKnnMaxK || N >= (int64_t(1) << 31) || B > 65535 || (kk > 0 && !cf_shape_ok(N, D))) return PPLIE_EUNSUPPORTED;
  if (kk > N) return PPLIE_EBADARG;
  if (B == 0 || N == 0) return PPLIE_OK;
  if (!pcount || !mask || (kk > 0 && (!pd2 || !pidx || !cloud || !out))) return PPLIE_EBADARG;
  NbrFinishArgs<T> a;
  a.pcount = static_cast<const int*>(pcount); a.pd2 = static_cast<const T*>(pd2); a.pidx = static_cast<const int*>(pidx);
  a.cloud = static_cast<const T*>(cloud); a.mask = static_cast<unsigned char*>(mask); a.out = static_cast<T*>(out);
  a.N = N; a.D = D; a.kk = kk; a.S = S; a.nbr = nbr;
  const dim3 grid((unsigned)((N + kCfBlock - 1) / kCfBlock), (unsigned)B), block(kCfBlock);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  switch (kk == 0 ? 0 : knn_width(kk)) {
    case 0: hipLaunchKernelGGL((nbr_finish_kernel<T, 0>), grid, block, 0, st, a); break;
    case 1: hipLaunchKernelGGL((nbr_finish_kernel<T, 1>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((nbr_finish_kernel<T, 2>), grid, block, 0, st, a); break;
    case 4: hipLaunchKernelGGL((nbr_finish_kernel<T, 4>), grid, block, 0, st, a); break;
    case 8: hipLaunchKernelGGL((nbr_finish_kernel<T, 8>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((nbr_finish_kernel<T, 16>), grid, block, 0, st, a); break;
  }
  return knn_status();
}

template <class T>
int launch_voxel_keys(const void* cloud, int64_t N, int D, double v0, double v1, double v2, void* part, void* keys, void* flag,
                      void* stream) {
  if (N < 0 || !(v0 > 0) || !(v1 > 0) || !(v2 > 0)) return PPLIE_EBADARG;
  if (!cf_shape_ok(N, D)) return PPLIE_EUNSUPPORTED;
  if (N == 0) return PPLIE_OK;
  if (!cloud || !part || !keys || !flag) return PPLIE_EBADARG;
  const int64_t nwg = (N + kCfBlock - 1) / kCfBlock;
  const int npart = (int)(nwg < kCfMinParts ? nwg : kCfMinParts);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL((voxel_min_kernel<T>), dim3((unsigned)npart), dim3(kCfBlock), 0, st, static_cast<const T*>(cloud), N, D,
                     static_cast<T*>(part));
  hipLaunchKernelGGL((voxel_keys_kernel<T>), dim3((unsigned)nwg), dim3(kCfBlock), 0, st, static_cast<const T*>(cloud), N, D,
                     static_cast<const T*>(part), npart, (T)v0, (T)v1, (T)v2, static_cast<int64_t*>(keys), static_cast<int*>(flag));
  return knn_status();
}

inline int launch_voxel_heads(const void* keys, int64_t N, void* heads, void* stream) {
  if (N < 0) return PPLIE_EBADARG;
  if (N >= (int64_t(1) << 31)) return PPLIE_EUNSUPPORTED;
  if (N == 0) return PPLIE_OK;
  if (!keys || !heads) return PPLIE_EBADARG;
  hipLaunchKernelGGL(voxel_heads_kernel, dim3((unsigned)((N + kCfBlock - 1) / kCfBlock)), dim3(kCfBlock), 0,
                     reinterpret_cast<hipStream_t>(stream), static_cast<const int64_t*>(keys), N, static_cast<int*>(heads));
  return knn_status();
}

template <class T>
int launch_voxel_reduce(const void* keys, const void* perm, const void* cloud, const void* base, void* lead, void* tail, void* info,
                        void* out, void* start, void* count, int64_t N, int D, void* stream) {
  if (N < 0) return PPLIE_EBADARG;
  if (!cf_shape_ok(N, D)) return PPLIE_EUNSUPPORTED;
  if (N == 0) return PPLIE_OK;
  if (!keys || !perm || !cloud || !base || !lead || !tail || !info || !out || !start || !count) return PPLIE_EBADARG;
  VoxelReduceArgs<T> a;
  a.keys = static_cast<const int64_t*>(keys); a.perm = static_cast<const int64_t*>(perm); a.cloud = static_cast<const T*>(cloud);
  a.base = static_cast<const int64_t*>(base); a.lead = static_cast<double*>(lead); a.tail = static_cast<double*>(tail);
  a.info = static_cast<int*>(info); a.out = static_cast<T*>(out); a.start = static_cast<int*>(start);
  a.count = static_cast<int*>(count); a.N = N; a.D = D;
  const int64_t nwg = (N + kCfBlock - 1) / kCfBlock;
  a.nwg = (int)nwg;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL((voxel_reduce_kernel<T>), dim3((unsigned)nwg), dim3(kCfBlock), 0, st, a);
  hipLaunchKernelGGL((voxel_stitch_kernel<T>), dim3((unsigned)((nwg * kCfCols + kCfBlock - 1) / kCfBlock)), dim3(kCfBlock), 0, st, a);
  return knn_status();
}

}  // namespace pplie

#define PPLIE_CLOUD_FILTER_ENTRIES(SFX, T)                                                                                              \
  extern "C" int pplie_nbr_partial_##SFX(const void* pts, void* pcount, void* pd2, void* pidx, int64_t B, int64_t N, double r2,        \
                                         int kk, int S, void* stream) {                                                                \
    return pplie::launch_nbr_partial<T>(pts, pcount, pd2, pidx, B, N, r2, kk, S, stream);                                               \
  }                                                                                                                                     \
  extern "C" int pplie_nbr_finish_##SFX(const void* pcount, const void* pd2, const void* pidx, const void* cloud, void* mask,          \
                                        void* out, int64_t B, int64_t N, int D, int kk, int S, int nbr, void* stream) {                \
    return pplie::launch_nbr_finish<T>(pcount, pd2, pidx, cloud, mask, out, B, N, D, kk, S, nbr, stream);                               \
  }                                                                                                                                     \
  extern "C" int pplie_voxel_keys_##SFX(const void* cloud, int64_t N, int D, double v0, double v1, double v2, void* part, void* keys,  \
                                        void* flag, void* stream) {                                                                    \
    return pplie::launch_voxel_keys<T>(cloud, N, D, v0, v1, v2, part, keys, flag, stream);                                              \
  }                                                                                                                                     \
  extern "C" int pplie_voxel_reduce_##SFX(const void* keys, const void* perm, const void* cloud, const void* base, void* lead,         \
                                          void* tail, void* info, void* out, void* start, void* count, int64_t N, int D,               \
                                          void* stream) {                                                                              \
    return pplie::launch_voxel_reduce<T>(keys, perm, cloud, base, lead, tail, info, out, start, count, N, D, stream);                   \
  }
PPLIE_CLOUD_FILTER_ENTRIES(f32, float)
PPLIE_CLOUD_FILTER_ENTRIES(f64, double)
extern "C" int pplie_voxel_heads(const void* keys, int64_t N, void* heads, void* stream) {
  return pplie::launch_voxel_heads(keys, N, heads, stream);
}

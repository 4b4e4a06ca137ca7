// pnp_math.h -- the arithmetic of EPnP (camera pose from 3D-2D matches; reference pypose/module/pnp.py) for ONE problem, written
// against a small "context" that says how many lanes cooperate on the problem and how they add up and synchronise:
//
//   cx.lane(), cx.nl()      this lane among the nl lanes that walk the points
//   cx.reduce(v, n)         add v[0..n) over those lanes; the totals are in cx.red[0..n), visible to every lane on return
//   cx.dense()              this lane belongs to the group that runs the 12 x 12 eigenproblem (wave 0 of the problem)
//   cx.dlane(), cx.dn()     ... its index in that group and the group's size
//   cx.dsync()              barrier of that group;  cx.sync(): barrier of all lanes of the problem
//   cx.A, cx.V [144], cx.rot [12], cx.red [kPnpRed], cx.nv [48]     shared storage of the problem (LDS on the device)
//
// csrc/epnp.hip supplies a one-wavefront context (DPP sums, no workgroup barrier) and a one-workgroup context; a serial context
// with nl = dn = 1 runs the very same code on the host (tests/hostmath/pnp_check.cpp -- test infrastructure, never a product path).
// Everything here computes in fp64 whatever the type of the inputs: the work per problem is a few thousand flops per point pass
// and one 12 x 12 eigenproblem, the inputs' own rounding is then the only fp32 error, and the eigenvectors of the four SMALLEST
// eigenvalues of a matrix whose largest is ~1e8 times theirs are not something fp32 can deliver.
//
// The small dense pieces (symmetric 3 x 3 Jacobi, one-sided-Jacobi 3 x 3 SVD, Kabsch, Householder least squares / minimum norm,
// the beta rules) are plain functions on local arrays: every lane computes them redundantly from the same shared numbers, so
// there is nothing to broadcast and no divergence.  They are kept free of the context so that other kernels can use them.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PNP_HD __host__ __device__ __forceinline__
#else
#define PNP_HD inline
#endif

namespace pplie {
namespace pnp {

typedef double R;
enum { kPnpRed = 40, kPnpSweeps12 = 10, kPnpSweeps3 = 8 };

PNP_HD R sgn(R x) { return R((x > 0) - (x < 0)); }

// the rotation J = [[c, s], [-s, c]] that zeroes the (p, q) entry of J^T A J for a symmetric A
PNP_HD void sym_rot(R app, R aqq, R apq, R& c, R& s) {
  c = 1; s = 0;
  if (apq == 0) return;
  const R tau = (aqq - app) / (2 * apq);
  const R t = (tau >= 0 ? R(1) : R(-1)) / (fabs(tau) + sqrt(1 + tau * tau));
  c = 1 / sqrt(1 + t * t);
  s = t * c;
}

// ---- symmetric 3 x 3: eigenvalues w (descending) and eigenvectors as the COLUMNS of E, cyclic Jacobi, fixed sweep count
PNP_HD void jacobi3(R a[3][3], R w[3], R E[3][3]) {
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) E[i][j] = i == j;
  for (int sw = 0; sw < kPnpSweeps3; ++sw)
    for (int pq = 0; pq < 3; ++pq) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
      R c, s;
      sym_rot(a[p][p], a[q][q], a[p][q], c, s);
      for (int i = 0; i < 3; ++i) {
        const R x = a[i][p], y = a[i][q];
        a[i][p] = c * x - s * y; a[i][q] = s * x + c * y;
        const R ex = E[i][p], ey = E[i][q];
        E[i][p] = c * ex - s * ey; E[i][q] = s * ex + c * ey;
      }
      for (int j = 0; j < 3; ++j) {
        const R x = a[p][j], y = a[q][j];
        a[p][j] = c * x - s * y; a[q][j] = s * x + c * y;
      }
    }
  for (int i = 0; i < 3; ++i) w[i] = a[i][i];
  for (int i = 0; i < 2; ++i)                      // sort descending (three elements: two passes of a bubble)
    for (int j = 0; j < 2 - i; ++j)
      if (w[j] < w[j + 1]) {
        const R t = w[j]; w[j] = w[j + 1]; w[j + 1] = t;
        for (int r = 0; r < 3; ++r) { const R e = E[r][j]; E[r][j] = E[r][j + 1]; E[r][j + 1] = e; }
      }
}

PNP_HD R det3(const R m[3][3]) {
  return m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
         m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}

// ---- right singular vectors of a symmetric positive semi-definite 3 x 3 WITH THE SIGNS LAPACK GIVES THEM.  The reference builds
// its control points from rows of V of torch.linalg.svd(scatter matrix), so its result depends on the sign each singular vector
// happens to get; with a handful of noisy matches a different sign pattern moves the estimate by whole pixels.  The signs are a
// property of the algorithm every LAPACK runs (gesdd and gesvd, reference and vendor builds agree): Householder bidiagonalisation
// (dgebd2 / dlarfg), then the implicit QR iteration on the bidiagonal (dbdsqr: direction choice, zero-shift and shifted sweeps,
// dlasv2 on 2 x 2 blocks), negative values flipped into V^T, sorted descending.  This is that algorithm for n = 3, tracking V^T only
// (U = V for this class of matrix).  Every loop is bounded: the iteration count is capped as dbdsqr caps it.
PNP_HD R sign_of(R a, R b) { return b >= 0 ? fabs(a) : -fabs(a); }      // Fortran SIGN(a, b) (b = -0.0 never decides a sign here)

PNP_HD void lartg(R f, R g, R& c, R& s, R& r) {
  if (g == 0) { c = 1; s = 0; r = f; }
  else if (f == 0) { c = 0; s = sign_of(1, g); r = fabs(g); }
  else { const R d = sqrt(f * f + g * g); c = fabs(f) / d; r = sign_of(d, f); s = g / r; }
}

// smaller singular value of [[f, g], [0, h]] (dlas2)
PNP_HD R las2_min(R f, R g, R h) {
  const R fa = fabs(f), ga = fabs(g), ha = fabs(h), mn = fa < ha ? fa : ha, mx = fa < ha ? ha : fa;
  if (mn == 0) return 0;
  if (ga < mx) {
    const R as = 1 + mn / mx, at = (mx - mn) / mx, au = (ga / mx) * (ga / mx);
    return mn * (2 / (sqrt(as * as + au) + sqrt(at * at + au)));
  }
  const R au = mx / ga;
  if (au == 0) return mn * mx / ga;
  const R as = 1 + mn / mx, at = (mx - mn) / mx, c = 1 / (sqrt(1 + (as * au) * (as * au)) + sqrt(1 + (at * au) * (at * au)));
  return 2 * ((mn * c) * au);
}

// SVD of [[f, g], [0, h]] (dlasv2): signed values and the right rotation (csr, snr); the left one is not needed here
PNP_HD void lasv2(R f, R g, R h, R& ssmin, R& ssmax, R& snr, R& csr) {
  const R eps = 1.1102230246251565e-16;
  R ft = f, fa = fabs(f), ht = h, ha = fabs(h), clt, crt, slt, srt;
  int pmax = 1;
  const bool swap = ha > fa;
  if (swap) { pmax = 3; R t = ft; ft = ht; ht = t; t = fa; fa = ha; ha = t; }
  const R gt = g, ga = fabs(g);
  if (ga == 0) { ssmin = ha; ssmax = fa; clt = 1; crt = 1; slt = 0; srt = 0; }
  else {
    bool gasmal = true;
    if (ga > fa) {
      pmax = 2;
      if (fa / ga < eps) {
        gasmal = false;
        ssmax = ga;
        ssmin = ha > 1 ? fa / (ga / ha) : (fa / ga) * ha;
        clt = 1; slt = ht / gt; srt = 1; crt = ft / gt;
      }
    }
    if (gasmal) {
      const R d = fa - ha, l = d == fa ? R(1) : d / fa, m = gt / ft, mm = m * m;
      R t = 2 - l;
      const R s = sqrt(t * t + mm), r = l == 0 ? fabs(m) : sqrt(l * l + mm), a = 0.5 * (s + r);
      ssmin = ha / a; ssmax = fa * a;
      if (mm == 0) t = l == 0 ? sign_of(2, ft) * sign_of(1, gt) : gt / sign_of(d, ft) + m / t;
      else t = (m / (s + t) + m / (r + l)) * (1 + a);
      const R ll = sqrt(t * t + 4);
      crt = 2 / ll; srt = t / ll; clt = (crt + srt * m) / a; slt = (ht / ft) * srt / a;
    }
  }
  R csl, snl;
  if (swap) { csl = srt; snl = crt; csr = slt; snr = clt; } else { csl = clt; snl = slt; csr = crt; snr = srt; }
  const R tsign = pmax == 1 ? sign_of(1, csr) * sign_of(1, csl) * sign_of(1, f)
                : pmax == 2 ? sign_of(1, snr) * sign_of(1, csl) * sign_of(1, g) : sign_of(1, snr) * sign_of(1, snl) * sign_of(1, h);
  ssmax = sign_of(ssmax, tsign);
  ssmin = sign_of(ssmin, tsign * sign_of(1, f) * sign_of(1, h));
}

// rows j, j + 1 of VT <- plane rotation (dlasr 'L', 'V'): row j+1 = c row j+1 - s row j, row j = s row j+1 + c row j
PNP_HD void rot_rows(R VT[3][3], int j, R c, R s) {
  for (int x = 0; x < 3; ++x) {
    const R t = VT[j + 1][x];
    VT[j + 1][x] = c * t - s * VT[j][x];
    VT[j][x] = s * t + c * VT[j][x];
  }
}

// w: singular values descending; V: row j, column k = component j of the k-th right singular vector (V = VT^T)
PNP_HD void svd3_psd_lapack_signs(const R S[3][3], R w[3], R V[3][3]) {
  const R eps = 1.1102230246251565e-16, unfl = 2.2250738585072014e-308;
  R A[3][3], VT[3][3], d[3], e[2];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { A[i][j] = S[i][j]; VT[i][j] = i == j; }
  // dgebd2: H1 from the left on column 0, G1 from the right on row 0 (columns 1, 2), H2 from the left on column 1 (rows 1, 2)
  {
    const R xn = sqrt(A[1][0] * A[1][0] + A[2][0] * A[2][0]);
    if (xn != 0) {
      const R alpha = A[0][0], beta = -sign_of(sqrt(alpha * alpha + xn * xn), alpha), tau = (beta - alpha) / beta;
      const R v1 = A[1][0] / (alpha - beta), v2 = A[2][0] / (alpha - beta);
      for (int j = 1; j < 3; ++j) {
        const R dot = tau * (A[0][j] + v1 * A[1][j] + v2 * A[2][j]);
        A[0][j] -= dot; A[1][j] -= dot * v1; A[2][j] -= dot * v2;
      }
      A[0][0] = beta;
    }
    d[0] = A[0][0];
  }
  {
    const R xn = fabs(A[0][2]);
    if (xn != 0) {
      const R alpha = A[0][1], beta = -sign_of(sqrt(alpha * alpha + xn * xn), alpha), tau = (beta - alpha) / beta, v = A[0][2] / (alpha - beta);
      for (int i = 1; i < 3; ++i) {
        const R dot = tau * (A[i][1] + v * A[i][2]);
        A[i][1] -= dot; A[i][2] -= dot * v;
      }
      A[0][1] = beta;
      VT[1][1] = 1 - tau; VT[1][2] = VT[2][1] = -tau * v; VT[2][2] = 1 - tau * v * v;       // P^T = G1 (symmetric)
    }
    e[0] = A[0][1];
  }
  {
    const R xn = fabs(A[2][1]);
    if (xn != 0) {
      const R alpha = A[1][1], beta = -sign_of(sqrt(alpha * alpha + xn * xn), alpha), tau = (beta - alpha) / beta, v = A[2][1] / (alpha - beta);
      const R dot = tau * (A[1][2] + v * A[2][2]);
      A[1][2] -= dot; A[2][2] -= dot * v;
      A[1][1] = beta;
    }
    d[1] = A[1][1]; e[1] = A[1][2]; d[2] = A[2][2];
  }
  // dbdsqr, upper bidiagonal, n = 3 (indices 0-based; the block is ll..m)
  const R tolmul = fmax(R(10), fmin(R(100), pow(eps, R(-0.125)))), tol = tolmul * eps;
  R smax = fmax(fmax(fabs(d[0]), fabs(d[1])), fmax(fabs(d[2]), fmax(fabs(e[0]), fabs(e[1]))));
  R sminoa = fabs(d[0]), mu = sminoa, sminl = 0;
  for (int i = 1; i < 3 && sminoa != 0; ++i) { mu = fabs(d[i]) * (mu / (mu + fabs(e[i - 1]))); sminoa = fmin(sminoa, mu); }
  sminoa /= sqrt(R(3));
  const R thresh = fmax(tol * sminoa, R(6 * 3 * 3) * R(3 * 3) * unfl);
  int m = 2, oldll = -1, oldm = -1, idir = 0, iter = 0;
  for (int pass = 0; pass < 128 && m > 0 && iter <= 54; ++pass) {
    int ll = -1;
    bool split = false;
    smax = fabs(d[m]);
    for (int l = m - 1; l >= 0; --l) {
      if (fabs(e[l]) <= thresh) { e[l] = 0; ll = l; split = true; break; }
      smax = fmax(smax, fmax(fabs(d[l]), fabs(e[l])));
    }
    if (split && ll == m - 1) { --m; continue; }
    ll += 1;
    if (ll == m - 1) {                                     // 2 x 2 block
      R sigmn, sigmx, sinr, cosr;
      lasv2(d[m - 1], e[m - 1], d[m], sigmn, sigmx, sinr, cosr);
      d[m - 1] = sigmx; e[m - 1] = 0; d[m] = sigmn;
      for (int x = 0; x < 3; ++x) {                        // drot on rows m-1, m
        const R a = VT[m - 1][x], b = VT[m][x];
        VT[m - 1][x] = cosr * a + sinr * b; VT[m][x] = cosr * b - sinr * a;
      }
      m -= 2;
      continue;
    }
    if (ll > oldm || m < oldll) idir = fabs(d[ll]) >= fabs(d[m]) ? 1 : 2;
    bool again = false;
    if (idir == 1) {
      if (fabs(e[m - 1]) <= tol * fabs(d[m])) { e[m - 1] = 0; continue; }
      mu = fabs(d[ll]); sminl = mu;
      for (int l = ll; l < m; ++l) {
        if (fabs(e[l]) <= tol * mu) { e[l] = 0; again = true; break; }
        mu = fabs(d[l + 1]) * (mu / (mu + fabs(e[l]))); sminl = fmin(sminl, mu);
      }
    } else {
      if (fabs(e[ll]) <= tol * fabs(d[ll])) { e[ll] = 0; continue; }
      mu = fabs(d[m]); sminl = mu;
      for (int l = m - 1; l >= ll; --l) {
        if (fabs(e[l]) <= tol * mu) { e[l] = 0; again = true; break; }
        mu = fabs(d[l]) * (mu / (mu + fabs(e[l]))); sminl = fmin(sminl, mu);
      }
    }
    if (again) continue;
    oldll = ll; oldm = m;
    R shift = 0;
    if (!(3 * tol * (sminl / smax) <= fmax(eps, R(0.01) * tol))) {
      const R sll = idir == 1 ? fabs(d[ll]) : fabs(d[m]);
      shift = idir == 1 ? las2_min(d[m - 1], e[m - 1], d[m]) : las2_min(d[ll], e[ll], d[ll + 1]);
      if (sll > 0 && (shift / sll) * (shift / sll) < eps) shift = 0;
    }
    iter += m - ll;
    if (shift == 0) {
      if (idir == 1) {
        R cs = 1, oldcs = 1, sn = 0, oldsn = 0, r;
        for (int i = ll; i < m; ++i) {
          lartg(d[i] * cs, e[i], cs, sn, r);
          if (i > ll) e[i - 1] = oldsn * r;
          lartg(oldcs * r, d[i + 1] * sn, oldcs, oldsn, d[i]);
          rot_rows(VT, i, cs, sn);
        }
        const R h = d[m] * cs;
        d[m] = h * oldcs; e[m - 1] = h * oldsn;
        if (fabs(e[m - 1]) <= thresh) e[m - 1] = 0;
      } else {
        R cs = 1, oldcs = 1, sn = 0, oldsn = 0, r;
        for (int i = m; i > ll; --i) {
          lartg(d[i] * cs, e[i - 1], cs, sn, r);
          if (i < m) e[i] = oldsn * r;
          lartg(oldcs * r, d[i - 1] * sn, oldcs, oldsn, d[i]);
          rot_rows(VT, i - 1, oldcs, -oldsn);
        }
        const R h = d[ll] * cs;
        d[ll] = h * oldcs; e[ll] = h * oldsn;
        if (fabs(e[ll]) <= thresh) e[ll] = 0;
      }
    } else if (idir == 1) {
      R f = (fabs(d[ll]) - shift) * (sign_of(1, d[ll]) + shift / d[ll]), g = e[ll], cosr, sinr, cosl, sinl, r;
      for (int i = ll; i < m; ++i) {
        lartg(f, g, cosr, sinr, r);
        if (i > ll) e[i - 1] = r;
        f = cosr * d[i] + sinr * e[i]; e[i] = cosr * e[i] - sinr * d[i]; g = sinr * d[i + 1]; d[i + 1] = cosr * d[i + 1];
        lartg(f, g, cosl, sinl, r);
        d[i] = r;
        f = cosl * e[i] + sinl * d[i + 1]; d[i + 1] = cosl * d[i + 1] - sinl * e[i];
        if (i < m - 1) { g = sinl * e[i + 1]; e[i + 1] = cosl * e[i + 1]; }
        rot_rows(VT, i, cosr, sinr);
      }
      e[m - 1] = f;
      if (fabs(e[m - 1]) <= thresh) e[m - 1] = 0;
    } else {
      R f = (fabs(d[m]) - shift) * (sign_of(1, d[m]) + shift / d[m]), g = e[m - 1], cosr, sinr, cosl, sinl, r;
      for (int i = m; i > ll; --i) {
        lartg(f, g, cosr, sinr, r);
        if (i < m) e[i] = r;
        f = cosr * d[i] + sinr * e[i - 1]; e[i - 1] = cosr * e[i - 1] - sinr * d[i]; g = sinr * d[i - 1]; d[i - 1] = cosr * d[i - 1];
        lartg(f, g, cosl, sinl, r);
        d[i] = r;
        f = cosl * e[i - 1] + sinl * d[i - 1]; d[i - 1] = cosl * d[i - 1] - sinl * e[i - 1];
        if (i > ll + 1) { g = sinl * e[i - 2]; e[i - 2] = cosl * e[i - 2]; }
        rot_rows(VT, i - 1, cosl, -sinl);
      }
      e[ll] = f;
      if (fabs(e[ll]) <= thresh) e[ll] = 0;
    }
  }
  for (int i = 0; i < 3; ++i)
    if (d[i] < 0) { d[i] = -d[i]; for (int x = 0; x < 3; ++x) VT[i][x] = -VT[i][x]; }
  for (int i = 0; i < 2; ++i) {                            // dbdsqr's sort: the smallest of the unsorted part goes last
    int isub = 0;
    R smin = d[0];
    for (int j = 1; j < 3 - i; ++j) if (d[j] <= smin) { isub = j; smin = d[j]; }
    const int last = 2 - i;
    if (isub != last) {
      d[isub] = d[last]; d[last] = smin;
      for (int x = 0; x < 3; ++x) { const R t = VT[isub][x]; VT[isub][x] = VT[last][x]; VT[last][x] = t; }
    }
  }
  for (int k = 0; k < 3; ++k) { w[k] = d[k]; for (int j = 0; j < 3; ++j) V[j][k] = VT[k][j]; }
}

// ---- 3 x 3 SVD H = U diag(S) V^T by one-sided (Hestenes) Jacobi: the columns of H V are rotated until they are orthogonal; their
// lengths are the singular values (sorted descending).  A third column that vanished against the first (rank 2) has no direction of
// its own: it is completed as +-(u0 x u1), with the sign that keeps det(U) det(V) = +1.
PNP_HD void svd3(const R H[3][3], R U[3][3], R S[3], R V[3][3]) {
  R G[3][3];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { G[i][j] = H[i][j]; V[i][j] = i == j; }
  for (int sw = 0; sw < kPnpSweeps3; ++sw)
    for (int pq = 0; pq < 3; ++pq) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
      R al = 0, be = 0, ga = 0, c, s;
      for (int i = 0; i < 3; ++i) { al += G[i][p] * G[i][p]; be += G[i][q] * G[i][q]; ga += G[i][p] * G[i][q]; }
      sym_rot(al, be, ga, c, s);
      for (int i = 0; i < 3; ++i) {
        const R x = G[i][p], y = G[i][q];
        G[i][p] = c * x - s * y; G[i][q] = s * x + c * y;
        const R vx = V[i][p], vy = V[i][q];
        V[i][p] = c * vx - s * vy; V[i][q] = s * vx + c * vy;
      }
    }
  for (int j = 0; j < 3; ++j) S[j] = sqrt(G[0][j] * G[0][j] + G[1][j] * G[1][j] + G[2][j] * G[2][j]);
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2 - i; ++j)
      if (S[j] < S[j + 1]) {
        const R t = S[j]; S[j] = S[j + 1]; S[j + 1] = t;
        for (int r = 0; r < 3; ++r) {
          const R g = G[r][j]; G[r][j] = G[r][j + 1]; G[r][j + 1] = g;
          const R v = V[r][j]; V[r][j] = V[r][j + 1]; V[r][j + 1] = v;
        }
      }
  for (int j = 0; j < 2; ++j) for (int r = 0; r < 3; ++r) U[r][j] = G[r][j] / S[j];
  if (S[2] > 1e-14 * S[0]) {
    for (int r = 0; r < 3; ++r) U[r][2] = G[r][2] / S[2];
  } else {
    const R o = det3(V) < 0 ? R(-1) : R(1);
    U[0][2] = o * (U[1][0] * U[2][1] - U[2][0] * U[1][1]);
    U[1][2] = o * (U[2][0] * U[0][1] - U[0][0] * U[2][1]);
    U[2][2] = o * (U[0][0] * U[1][1] - U[1][0] * U[0][1]);
  }
}

// ---- Kabsch on the cross-covariance H = sum (q - qbar)(p - pbar)^T (q the target): Rm = U V^T, and svdtf's reflection rule
// (|det + 1| < 1e-6: Rm -> -Rm, reference function/geometry.py svdtf); t = qbar - Rm pbar
PNP_HD void kabsch(const R H[3][3], const R pbar[3], const R qbar[3], R Rm[3][3], R t[3]) {
  R U[3][3], S[3], V[3][3];
  svd3(H, U, S, V);
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Rm[i][j] = U[i][0] * V[j][0] + U[i][1] * V[j][1] + U[i][2] * V[j][2];
  if (fabs(det3(Rm) + 1) < 1e-6)
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Rm[i][j] = -Rm[i][j];
  for (int i = 0; i < 3; ++i) t[i] = qbar[i] - (Rm[i][0] * pbar[0] + Rm[i][1] * pbar[1] + Rm[i][2] * pbar[2]);
}

// rotation matrix -> unit quaternion xyzw (the largest of w, x, y, z is the pivot: no cancellation)
PNP_HD void rot2quat(const R m[3][3], R q[4]) {
  const R tr = m[0][0] + m[1][1] + m[2][2];
  if (tr >= m[0][0] && tr >= m[1][1] && tr >= m[2][2]) {
    const R s = 2 * sqrt(1 + tr);
    q[3] = s / 4; q[0] = (m[2][1] - m[1][2]) / s; q[1] = (m[0][2] - m[2][0]) / s; q[2] = (m[1][0] - m[0][1]) / s;
  } else if (m[0][0] >= m[1][1] && m[0][0] >= m[2][2]) {
    const R s = 2 * sqrt(1 + m[0][0] - m[1][1] - m[2][2]);
    q[3] = (m[2][1] - m[1][2]) / s; q[0] = s / 4; q[1] = (m[0][1] + m[1][0]) / s; q[2] = (m[0][2] + m[2][0]) / s;
  } else if (m[1][1] >= m[2][2]) {
    const R s = 2 * sqrt(1 + m[1][1] - m[0][0] - m[2][2]);
    q[3] = (m[0][2] - m[2][0]) / s; q[0] = (m[0][1] + m[1][0]) / s; q[1] = s / 4; q[2] = (m[1][2] + m[2][1]) / s;
  } else {
    const R s = 2 * sqrt(1 + m[2][2] - m[0][0] - m[1][1]);
    q[3] = (m[1][0] - m[0][1]) / s; q[0] = (m[0][2] + m[2][0]) / s; q[1] = (m[1][2] + m[2][1]) / s; q[2] = s / 4;
  }
  const R n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int i = 0; i < 4; ++i) q[i] /= n;
}

// ---- Householder QR of A [M][N] (row-major, M >= N) in place: R on and above the diagonal, the reflector vectors below it, their
// leading entries in vd, 2 / v^T v in tau (0: the column was already zero below the diagonal and the step is the identity)
template <int M, int N> PNP_HD void house_qr(R* A, R* vd, R* tau) {
  for (int k = 0; k < N; ++k) {
    R below = 0;
    for (int i = k + 1; i < M; ++i) below += A[i * N + k] * A[i * N + k];
    const R akk = A[k * N + k], norm = sqrt(akk * akk + below), alpha = akk > 0 ? -norm : norm;
    const R vk = akk - alpha, vtv = vk * vk + below;
    vd[k] = vk;
    tau[k] = vtv > 0 ? 2 / vtv : (vtv == 0 ? R(0) : vtv);          // (a NaN stays a NaN)
    for (int j = k + 1; j < N; ++j) {
      R dot = vk * A[k * N + j];
      for (int i = k + 1; i < M; ++i) dot += A[i * N + k] * A[i * N + j];
      dot *= tau[k];
      A[k * N + j] -= dot * vk;
      for (int i = k + 1; i < M; ++i) A[i * N + j] -= dot * A[i * N + k];
    }
    A[k * N + k] = alpha;
  }
}

// y <- H_k y for the k-th reflector of house_qr
template <int M, int N> PNP_HD void house_apply(const R* A, const R* vd, const R* tau, int k, R* y) {
  R dot = vd[k] * y[k];
  for (int i = k + 1; i < M; ++i) dot += A[i * N + k] * y[i];
  dot *= tau[k];
  y[k] -= dot * vd[k];
  for (int i = k + 1; i < M; ++i) y[i] -= dot * A[i * N + k];
}

// least squares x [N] = argmin |A x - b|, A [M][N] of full column rank, M >= N; A and b are overwritten
template <int M, int N> PNP_HD void house_lstsq(R* A, R* b, R* x) {
  R vd[N], tau[N];
  house_qr<M, N>(A, vd, tau);
  for (int k = 0; k < N; ++k) house_apply<M, N>(A, vd, tau, k, b);
  for (int i = N - 1; i >= 0; --i) {
    R acc = b[i];
    for (int j = i + 1; j < N; ++j) acc -= A[i * N + j] * x[j];
    x[i] = acc / A[i * N + i];
  }
}

// minimum-norm solution x [N] of the under-determined A x = b, A [M][N] of full row rank, M < N, by Householder on A^T:
// A^T = Q R1, R1^T y = b, x = Q [y; 0]
template <int M, int N> PNP_HD void house_minnorm(const R* A, const R* b, R* x) {
  R At[N * M], vd[M], tau[M];
  for (int i = 0; i < M; ++i) for (int j = 0; j < N; ++j) At[j * M + i] = A[i * N + j];
  house_qr<N, M>(At, vd, tau);
  for (int j = 0; j < N; ++j) x[j] = 0;
  for (int i = 0; i < M; ++i) {
    R acc = b[i];
    for (int j = 0; j < i; ++j) acc -= At[j * M + i] * x[j];
    x[i] = acc / At[i * M + i];
  }
  for (int k = M - 1; k >= 0; --k) house_apply<N, M>(At, vd, tau, k, x);
}

// ---- the four beta candidates (Eq. 10-14 of the EPnP paper, the reference's three least-squares cases and its sign rules) from
// L [6][10] and rho [6]; the columns of L are the products b_a b_b in the order 00 01 11 02 12 22 03 13 23 33
PNP_HD void betas_from_l(const R* L, const R* rho, R betas[4][4]) {
  for (int c = 0; c < 4; ++c) for (int i = 0; i < 4; ++i) betas[c][i] = 0;
  betas[0][3] = 1;
  {
    const int col[3] = {5, 8, 9};
    R A[18], b[6], S[3];
    for (int e = 0; e < 6; ++e) { b[e] = rho[e]; for (int j = 0; j < 3; ++j) A[e * 3 + j] = L[e * 10 + col[j]]; }
    house_lstsq<6, 3>(A, b, S);
    betas[1][2] = sqrt(fabs(S[0]));
    betas[1][3] = sqrt(fabs(S[2])) * sgn(S[1]) * sgn(S[0]);
  }
  {
    const int col[6] = {2, 4, 7, 5, 8, 9};
    R A[36], b[6], S[6];
    for (int e = 0; e < 6; ++e) { b[e] = rho[e]; for (int j = 0; j < 6; ++j) A[e * 6 + j] = L[e * 10 + col[j]]; }
    house_lstsq<6, 6>(A, b, S);
    betas[2][1] = sqrt(fabs(S[0]));
    betas[2][2] = sqrt(fabs(S[3])) * sgn(S[1]) * sgn(S[0]);
    betas[2][3] = sqrt(fabs(S[5])) * sgn(S[2]) * sgn(S[0]);
  }
  {
    R S[10];
    house_minnorm<6, 10>(L, rho, S);
    betas[3][0] = sqrt(fabs(S[9])) * sgn(S[6]) * sgn(S[0]);
    betas[3][1] = sqrt(fabs(S[5])) * sgn(S[3]) * sgn(S[0]);
    betas[3][2] = sqrt(fabs(S[2])) * sgn(S[1]) * sgn(S[0]);
    betas[3][3] = sqrt(fabs(S[0]));
  }
}

// ---- symmetric 12 x 12 eigenproblem A = V diag V^T by parallel-ordered cyclic Jacobi on shared storage.  A round applies the 6
// disjoint rotations of a round-robin pairing (player 11 stays, the other 11 turn), 11 rounds meet every pair once (a sweep), the
// sweep count is fixed.  Per round: 6 lanes form (c, s); 144 lane-items rotate the columns of A and V; 72 rotate the rows of A.
PNP_HD void jacobi12_pair(int r, int k, int& p, int& q) {
  if (k == 0) { p = r; q = 11; } else { p = (r + k) % 11; q = (r + 11 - k) % 11; }
}

template <class C> PNP_HD void jacobi12(C& cx, R* A, R* V, R* rot) {
  const int l = cx.dlane(), n = cx.dn();
  for (int i = l; i < 144; i += n) V[i] = (i / 12 == i % 12) ? R(1) : R(0);
  cx.dsync();
  for (int sw = 0; sw < kPnpSweeps12; ++sw)
    for (int r = 0; r < 11; ++r) {
      for (int k = l; k < 6; k += n) {
        int p, q;
        jacobi12_pair(r, k, p, q);
        sym_rot(A[p * 12 + p], A[q * 12 + q], A[p * 12 + q], rot[2 * k], rot[2 * k + 1]);
      }
      cx.dsync();
      for (int it = l; it < 144; it += n) {
        R* M = it < 72 ? A : V;
        const int i = (it % 72) / 6, k = it % 6;
        int p, q;
        jacobi12_pair(r, k, p, q);
        const R c = rot[2 * k], s = rot[2 * k + 1], x = M[i * 12 + p], y = M[i * 12 + q];
        M[i * 12 + p] = c * x - s * y; M[i * 12 + q] = s * x + c * y;
      }
      cx.dsync();
      for (int it = l; it < 72; it += n) {
        const int k = it / 12, j = it % 12;
        int p, q;
        jacobi12_pair(r, k, p, q);
        const R c = rot[2 * k], s = rot[2 * k + 1], x = A[p * 12 + j], y = A[q * 12 + j];
        A[p * 12 + j] = c * x - s * y; A[q * 12 + j] = s * x + c * y;
      }
      cx.dsync();
    }
}

// ---- one EPnP problem --------------------------------------------------------------------------------------------------------
// the control-point frame of the world cloud: centroid c0, orthonormal directions dir[j], spreads w[j] (descending)
struct Frame { R c0[3], dir[3][3], w[3], isq[3]; };
struct Camera { R K[9], fu, fv, u0, v0; };

PNP_HD void alphas(const Frame& f, const R p[3], R d[3], R a[3]) {
  for (int x = 0; x < 3; ++x) d[x] = p[x] - f.c0[x];
  for (int j = 0; j < 3; ++j) a[j] = (f.dir[j][0] * d[0] + f.dir[j][1] * d[1] + f.dir[j][2] * d[2]) * f.isq[j];
}

// the pairs (i, j) of control points whose six distances fix the betas
PNP_HD int pair_i(int e) { return e < 3 ? e + 1 : (e == 3 ? 2 : 3); }
PNP_HD int pair_j(int e) { return e < 3 ? 0 : (e == 5 ? 2 : 1); }

template <class T, class C> struct Solver {
  C& cx;
  const T* pts; const T* pix;
  int64_t N;
  Frame f;
  Camera cam;
  R P0[3], U0[2];          // this lane's first point: N <= nl never goes back to memory
  bool has0;

  PNP_HD Solver(C& c, const T* points, const T* pixels, const T* K, int64_t n) : cx(c), pts(points), pix(pixels), N(n) {
    for (int i = 0; i < 9; ++i) cam.K[i] = R(K[i]);
    cam.fu = cam.K[0]; cam.fv = cam.K[4]; cam.u0 = cam.K[2]; cam.v0 = cam.K[5];
    has0 = cx.lane() < N;
    for (int x = 0; x < 3; ++x) P0[x] = has0 ? R(pts[(int64_t)cx.lane() * 3 + x]) : R(0);
    for (int x = 0; x < 2; ++x) U0[x] = has0 ? R(pix[(int64_t)cx.lane() * 2 + x]) : R(0);
  }

  template <class F> PNP_HD void each_point(F&& fn) {
    if (has0) fn(P0, U0);
    for (int64_t i = (int64_t)cx.lane() + cx.nl(); i < N; i += cx.nl()) {
      const R p[3] = {R(pts[i * 3]), R(pts[i * 3 + 1]), R(pts[i * 3 + 2])}, u[2] = {R(pix[i * 2]), R(pix[i * 2 + 1])};
      fn(p, u);
    }
  }

  // stage 1: centroid, scatter matrix, its eigen-decomposition.  The reference scales ROW j of the eigenvector matrix by sqrt(s_j)
  // (pnp.py _svd_basis: s.sqrt().unsqueeze(-1) * vh.mT); the rows of an orthogonal matrix are as orthonormal as its columns, so the
  // closed-form barycentric weights hold for them too, and they are what is used here.  The signs of the singular vectors are LAPACK's
  // (svd3_psd_lapack_signs): another sign pattern is another control tetrahedron, and under pixel noise another estimate.
  PNP_HD bool control_points(R tol) {
    R v[6] = {0, 0, 0, 0, 0, 0};
    each_point([&](const R* p, const R*) { v[0] += p[0]; v[1] += p[1]; v[2] += p[2]; });
    cx.reduce(v, 3);
    for (int x = 0; x < 3; ++x) { f.c0[x] = cx.red[x] / R(N); v[x] = 0; }
    each_point([&](const R* p, const R*) {
      const R d[3] = {p[0] - f.c0[0], p[1] - f.c0[1], p[2] - f.c0[2]};
      v[0] += d[0] * d[0]; v[1] += d[0] * d[1]; v[2] += d[0] * d[2]; v[3] += d[1] * d[1]; v[4] += d[1] * d[2]; v[5] += d[2] * d[2];
    });
    cx.reduce(v, 6);
    R S[3][3] = {{cx.red[0], cx.red[1], cx.red[2]}, {cx.red[1], cx.red[3], cx.red[4]}, {cx.red[2], cx.red[4], cx.red[5]}}, E[3][3];
    svd3_psd_lapack_signs(S, f.w, E);
    R thin[3], unused[3][3];
    jacobi3(S, thin, unused);          // flatness is judged on Jacobi's values: relatively accurate where the QR iteration's are only absolutely so
    for (int j = 0; j < 3; ++j) {
      for (int x = 0; x < 3; ++x) f.dir[j][x] = E[j][x];
      f.isq[j] = 1 / sqrt(f.w[j]);
    }
    return thin[2] > tol * thin[0];
  }

  // stages 2-4: the 40 sums of M^T M, the 12 x 12 matrix in shared storage, its eigenvectors, the four of the smallest
  // eigenvalues as cx.nv [4][12] in the reference's order (the smallest last)
  PNP_HD void null_vectors() {
    R v[kPnpRed];
    for (int i = 0; i < kPnpRed; ++i) v[i] = 0;
    each_point([&](const R* p, const R* u) {
      R d[3], a[4];
      alphas(f, p, d, a + 1);
      a[0] = 1 - (a[1] + a[2] + a[3]);
      const R du = cam.u0 - u[0], dv = cam.v0 - u[1], g = du * du + dv * dv;
      int m = 0;
      for (int j = 0; j < 4; ++j)
        for (int k = j; k < 4; ++k, m += 4) {
          const R aa = a[j] * a[k];
          v[m] += aa; v[m + 1] += aa * du; v[m + 2] += aa * dv; v[m + 3] += aa * g;
        }
    });
    cx.reduce(v, kPnpRed);
    if (cx.dense()) {
      for (int it = cx.dlane(); it < 144; it += cx.dn()) {
        const int row = it / 12, col = it % 12, j = row / 3, a = row % 3, k = col / 3, b = col % 3;
        const int lo = j < k ? j : k, hi = j < k ? k : j;
        const R* s = cx.red + 4 * (lo * 4 - lo * (lo - 1) / 2 + hi - lo);
        R val = 0;
        if (a == 0 && b == 0) val = cam.fu * cam.fu * s[0];
        else if (a == 1 && b == 1) val = cam.fv * cam.fv * s[0];
        else if (a == 2 && b == 2) val = s[3];
        else if (a + b == 2) val = cam.fu * s[1];         // (0, 2), (2, 0)
        else if (a + b == 3) val = cam.fv * s[2];         // (1, 2), (2, 1)
        cx.A[it] = val;
      }
      cx.dsync();
      jacobi12(cx, cx.A, cx.V, cx.rot);
      int idx[4];
      for (int m = 0; m < 4; ++m) {
        int best = -1;
        R bv = 0;
        for (int i = 0; i < 12; ++i) {
          bool taken = false;
          for (int t = 0; t < m; ++t) taken = taken || idx[t] == i;
          const R e = cx.A[i * 13];
          if (!taken && (best < 0 || e < bv)) { best = i; bv = e; }
        }
        idx[m] = best;
      }
      for (int it = cx.dlane(); it < 48; it += cx.dn()) cx.nv[it] = cx.V[(it % 12) * 12 + idx[3 - it / 12]];
    }
    cx.sync();
  }

  // stage 5
  PNP_HD void beta_candidates(R betas[4][4]) {
    const int ca[10] = {0, 0, 1, 0, 1, 2, 0, 1, 2, 3}, cb[10] = {0, 1, 1, 2, 2, 2, 3, 3, 3, 3};
    R L[60], rho[6];
    for (int e = 0; e < 6; ++e) {
      const int i = pair_i(e), j = pair_j(e);
      R dv[4][3], acc = 0;
      for (int a = 0; a < 4; ++a) for (int x = 0; x < 3; ++x) dv[a][x] = cx.nv[a * 12 + 3 * i + x] - cx.nv[a * 12 + 3 * j + x];
      for (int m = 0; m < 10; ++m) {
        const R* A = dv[ca[m]]; const R* B = dv[cb[m]];
        L[e * 10 + m] = (A[0] * B[0] + A[1] * B[1] + A[2] * B[2]) * (ca[m] == cb[m] ? R(1) : R(2));
      }
      for (int x = 0; x < 3; ++x) {                        // |bases_i - bases_j|^2, bases_0 = c0, bases_j = c0 + sqrt(w_j) dir_j
        const R bi = sqrt(f.w[i - 1]) * f.dir[i - 1][x], bj = j ? sqrt(f.w[j - 1]) * f.dir[j - 1][x] : R(0);
        acc += (bi - bj) * (bi - bj);
      }
      rho[e] = acc;
    }
    betas_from_l(L, rho, betas);
  }

  // stage 6 for one beta: camera-frame points alpha . C, the reference's scale and its flip on any negative z, Kabsch, the mean
  // reprojection error.  Everything is centred on the control frame: alpha_0 = 1 - sum alpha_j makes p_cam - C_0 = sum_j alpha_j
  // (C_j - C_0), and the world cloud is centred on c0, so the cross-covariance has no large terms to cancel.
  PNP_HD void evaluate(const R beta[4], R pose[7], R& err, R& scale) {
    R Cc[4][3], D[3][3];
    for (int j = 0; j < 4; ++j)
      for (int x = 0; x < 3; ++x) {
        R acc = 0;
        for (int a = 0; a < 4; ++a) acc += beta[a] * cx.nv[a * 12 + 3 * j + x];
        Cc[j][x] = acc;
      }
    for (int j = 0; j < 3; ++j) for (int x = 0; x < 3; ++x) D[j][x] = Cc[j + 1][x] - Cc[0][x];
    R v[12];
    for (int i = 0; i < 12; ++i) v[i] = 0;
    each_point([&](const R* p, const R*) {
      R d[3], a[3], q[3];
      alphas(f, p, d, a);
      for (int x = 0; x < 3; ++x) q[x] = a[0] * D[0][x] + a[1] * D[1][x] + a[2] * D[2][x];
      const R dc2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2], dw2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
      v[0] += sqrt(dc2) * sqrt(dw2); v[1] += dc2; v[2] += Cc[0][2] + q[2] < 0 ? R(1) : R(0);
      for (int x = 0; x < 3; ++x) for (int y = 0; y < 3; ++y) v[3 + 3 * x + y] += q[x] * d[y];
    });
    cx.reduce(v, 12);
    const R s0 = cx.red[0] / cx.red[1];                                   // >= 0: the flip can test the unscaled z
    scale = (cx.red[2] > 0 && s0 > 0) ? -s0 : s0;
    R H[3][3], qbar[3], Rm[3][3], t[3];
    for (int x = 0; x < 3; ++x) for (int y = 0; y < 3; ++y) H[x][y] = cx.red[3 + 3 * x + y];
    for (int x = 0; x < 3; ++x) { qbar[x] = scale * Cc[0][x]; for (int y = 0; y < 3; ++y) H[x][y] *= scale; }
    kabsch(H, f.c0, qbar, Rm, t);
    R e[1] = {0};
    each_point([&](const R* p, const R* u) {
      R c[3], h[3];
      for (int x = 0; x < 3; ++x) c[x] = Rm[x][0] * p[0] + Rm[x][1] * p[1] + Rm[x][2] * p[2] + t[x];
      for (int x = 0; x < 3; ++x) h[x] = cam.K[3 * x] * c[0] + cam.K[3 * x + 1] * c[1] + cam.K[3 * x + 2] * c[2];
      const R wabs = fabs(h[2]) > 2.2250738585072014e-308 ? fabs(h[2]) : 2.2250738585072014e-308, w = h[2] < 0 ? -wabs : wabs;
      const R ex = h[0] / w - u[0], ey = h[1] / w - u[1];
      e[0] += sqrt(ex * ex + ey * ey);
    });
    cx.reduce(e, 1);
    err = cx.red[0] / R(N);
    for (int x = 0; x < 3; ++x) pose[x] = t[x];
    rot2quat(Rm, pose + 3);
  }

  // stage 7: Gauss-Newton on the four betas against the six control-point distances; a fixed number of steps, the best iterate
  // is kept.  Each problem on its own: nothing here sees another problem of the batch.
  PNP_HD R distance_residual(const R beta[4], R e[6], R J[24]) {
    R loss = 0;
    for (int k = 0; k < 6; ++k) {
      const int i = pair_i(k), j = pair_j(k);
      R dv[4][3], diff[3] = {0, 0, 0}, bw = 0;
      for (int a = 0; a < 4; ++a)
        for (int x = 0; x < 3; ++x) {
          dv[a][x] = cx.nv[a * 12 + 3 * i + x] - cx.nv[a * 12 + 3 * j + x];
          diff[x] += beta[a] * dv[a][x];
        }
      for (int x = 0; x < 3; ++x) {
        const R bi = sqrt(f.w[i - 1]) * f.dir[i - 1][x], bj = j ? sqrt(f.w[j - 1]) * f.dir[j - 1][x] : R(0);
        bw += (bi - bj) * (bi - bj);
      }
      const R dc = sqrt(diff[0] * diff[0] + diff[1] * diff[1] + diff[2] * diff[2]);
      e[k] = sqrt(bw) - dc;
      for (int a = 0; a < 4; ++a) J[k * 4 + a] = -(diff[0] * dv[a][0] + diff[1] * dv[a][1] + diff[2] * dv[a][2]) / dc;
      loss += e[k] * e[k];
    }
    return loss;
  }

  PNP_HD void refine(R beta[4], int steps) {
    R cur[4] = {beta[0], beta[1], beta[2], beta[3]}, e[6], J[24], step[4];
    R best = distance_residual(cur, e, J);
    for (int s = 0; s < steps; ++s) {
      for (int k = 0; k < 6; ++k) e[k] = -e[k];
      house_lstsq<6, 4>(J, e, step);
      for (int a = 0; a < 4; ++a) cur[a] += step[a];
      const R loss = distance_residual(cur, e, J);
      if (loss < best) { best = loss; for (int a = 0; a < 4; ++a) beta[a] = cur[a]; }
    }
  }

  // the whole problem; pose [7] = translation, quaternion xyzw, all NaN for a degenerate or non-finite problem
  PNP_HD void solve(int refine_steps, R tol, R pose[7]) {
    const R nan = R(NAN);
    const bool ok = control_points(tol);
    null_vectors();
    R betas[4][4], best_err = R(INFINITY), best_beta[4] = {nan, nan, nan, nan}, best_scale = nan;
    for (int i = 0; i < 7; ++i) pose[i] = nan;
    beta_candidates(betas);
    for (int c = 0; c < 4; ++c) {
      R cand[7], err, scale;
      evaluate(betas[c], cand, err, scale);
      if (err < best_err) {
        best_err = err; best_scale = scale;
        for (int i = 0; i < 7; ++i) pose[i] = cand[i];
        for (int a = 0; a < 4; ++a) best_beta[a] = betas[c][a];
      }
    }
    if (refine_steps > 0) {
      R err, scale;
      for (int a = 0; a < 4; ++a) best_beta[a] *= best_scale;
      refine(best_beta, refine_steps);
      evaluate(best_beta, pose, err, scale);
    }
    bool finite = ok;
    for (int i = 0; i < 7; ++i) finite = finite && fabs(pose[i]) <= 1.7976931348623157e308;
    if (!finite) for (int i = 0; i < 7; ++i) pose[i] = nan;
  }
};

}  // namespace pnp
}  // namespace pplie

// pnp_check.cpp -- csrc/pnp_math.h compiled for the host and held to LAPACK-free identities (test infrastructure only):
//   Jacobi 12 x 12 and 3 x 3, the LAPACK-ordered 3 x 3:  |A V - V diag| and |V^T V - I|;   3 x 3 SVD: |U S V^T - H|, orthogonality, a rank-2 matrix;
//   Kabsch: det R = +1 and the planted rotation back;   least squares / minimum norm: normal equations and A x = b;
//   one EPnP problem end to end through the serial context (the code the kernel runs, one lane).
// Built and run by tests/test_pnp_host.py, once plain and once with -fsanitize=address,undefined.  Exit status 0 = all held.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pnp_math.h"

using namespace pplie::pnp;

struct SerialContext {
  R A[144], V[144], rot[12], red[kPnpRed], nv[48];
  int lane() const { return 0; }
  int nl() const { return 1; }
  bool dense() const { return true; }
  int dlane() const { return 0; }
  int dn() const { return 1; }
  void dsync() {}
  void sync() {}
  void reduce(const R* v, int n) { for (int i = 0; i < n; ++i) red[i] = v[i]; }
};

static unsigned long long g_state = 88172645463325252ull;
static double uniform() {                       // xorshift64: the same numbers everywhere
  g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
  return double(g_state >> 11) / 9007199254740992.0 * 2 - 1;
}

static int g_failed = 0;
static void hold(const char* what, double got, double bound) {
  std::printf("%-44s %.3e (bound %.1e)%s\n", what, got, bound, got <= bound ? "" : "   <-- FAILED");
  if (!(got <= bound)) g_failed = 1;
}

static void random_rotation(R Rm[3][3]) {
  R q[4], n = 0;
  for (int i = 0; i < 4; ++i) { q[i] = uniform(); n += q[i] * q[i]; }
  for (int i = 0; i < 4; ++i) q[i] /= std::sqrt(n);
  const R x = q[0], y = q[1], z = q[2], w = q[3];
  const R m[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                     {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                     {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Rm[i][j] = m[i][j];
}

static void check_jacobi12() {
  SerialContext cx;
  R B[12 * 20], A0[144];
  double resid = 0, orth = 0, scale = 0;
  for (int trial = 0; trial < 20; ++trial) {
    // a Gram matrix with columns graded over eight decades: large and tiny eigenvalues together, as M^T M has them
    for (int i = 0; i < 12 * 20; ++i) B[i] = uniform() * std::pow(10.0, -(i % 12) * 8.0 / 11);
    for (int i = 0; i < 12; ++i)
      for (int j = 0; j < 12; ++j) {
        R acc = 0;
        for (int k = 0; k < 20; ++k) acc += B[k * 12 + i] * B[k * 12 + j];
        cx.A[i * 12 + j] = A0[i * 12 + j] = acc;
        scale = std::fmax(scale, std::fabs(acc));
      }
    jacobi12(cx, cx.A, cx.V, cx.rot);
    for (int i = 0; i < 12; ++i)
      for (int j = 0; j < 12; ++j) {
        R av = 0, vv = 0;
        for (int k = 0; k < 12; ++k) { av += A0[i * 12 + k] * cx.V[k * 12 + j]; vv += cx.V[k * 12 + i] * cx.V[k * 12 + j]; }
        resid = std::fmax(resid, std::fabs(av - cx.V[i * 12 + j] * cx.A[j * 13]));
        orth = std::fmax(orth, std::fabs(vv - (i == j)));
      }
  }
  hold("jacobi12 |A V - V diag| / |A|", resid / scale, 1e-14);
  hold("jacobi12 |V^T V - I|", orth, 1e-14);
}

static void check_small() {
  double eig = 0, eorth = 0, rec = 0, sorth = 0, rot = 0, det = 0, order = 0, lap = 0;
  for (int trial = 0; trial < 200; ++trial) {
    R H[3][3], Sy[3][3], S0[3][3], w[3], E[3][3], U[3][3], S[3], V[3][3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) H[i][j] = uniform();
    if (trial % 4 == 1) for (int i = 0; i < 3; ++i) H[i][2] = H[i][0] - 2 * H[i][1];          // rank 2
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Sy[i][j] = S0[i][j] = H[0][i] * H[0][j] + H[1][i] * H[1][j] + H[2][i] * H[2][j];
    R wl[3], Vl[3][3];
    svd3_psd_lapack_signs(S0, wl, Vl);               // the LAPACK-ordered SVD of the same matrix: S V = V diag, V^T V = I
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        R av = 0, vv = 0;
        for (int k = 0; k < 3; ++k) { av += S0[i][k] * Vl[k][j]; vv += Vl[k][i] * Vl[k][j]; }
        lap = std::fmax(lap, std::fmax(std::fabs(av - Vl[i][j] * wl[j]), std::fabs(vv - (i == j))));
      }
    jacobi3(Sy, w, E);
    lap = std::fmax(lap, std::fmax(std::fabs(w[0] - wl[0]), std::fmax(std::fabs(w[1] - wl[1]), std::fabs(w[2] - wl[2]))));
    svd3(H, U, S, V);
    order = std::fmax(order, std::fmax(std::fmax(w[1] - w[0], w[2] - w[1]), std::fmax(S[1] - S[0], S[2] - S[1])));
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        R av = 0, ee = 0, usv = 0, uu = 0, vv = 0;
        for (int k = 0; k < 3; ++k) {
          av += S0[i][k] * E[k][j]; ee += E[k][i] * E[k][j]; usv += U[i][k] * S[k] * V[j][k];
          uu += U[k][i] * U[k][j]; vv += V[k][i] * V[k][j];
        }
        eig = std::fmax(eig, std::fabs(av - E[i][j] * w[j]));
        eorth = std::fmax(eorth, std::fabs(ee - (i == j)));
        rec = std::fmax(rec, std::fabs(usv - H[i][j]));
        sorth = std::fmax(sorth, std::fmax(std::fabs(uu - (i == j)), std::fabs(vv - (i == j))));
      }
    // Kabsch: q = Rt p + tt for a centred cloud p (a flat one every fourth trial), H = sum q p^T
    R Rt[3][3], P[8][3], Hk[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, pbar[3] = {0, 0, 0}, qbar[3], Rm[3][3], t[3];
    const R tt[3] = {uniform() * 5, uniform() * 5, uniform() * 5};
    random_rotation(Rt);
    for (int n = 0; n < 8; ++n) for (int x = 0; x < 3; ++x) { P[n][x] = (x == 2 && trial % 4 == 2) ? 0 : uniform(); pbar[x] += P[n][x] / 8; }
    for (int n = 0; n < 8; ++n)
      for (int x = 0; x < 3; ++x)
        for (int y = 0; y < 3; ++y)
          Hk[x][y] += (Rt[x][0] * (P[n][0] - pbar[0]) + Rt[x][1] * (P[n][1] - pbar[1]) + Rt[x][2] * (P[n][2] - pbar[2])) * (P[n][y] - pbar[y]);
    for (int x = 0; x < 3; ++x) qbar[x] = Rt[x][0] * pbar[0] + Rt[x][1] * pbar[1] + Rt[x][2] * pbar[2] + tt[x];
    kabsch(Hk, pbar, qbar, Rm, t);
    det = std::fmax(det, std::fabs(det3(Rm) - 1));
    for (int i = 0; i < 3; ++i) {
      rot = std::fmax(rot, std::fabs(t[i] - tt[i]));
      for (int j = 0; j < 3; ++j) rot = std::fmax(rot, std::fabs(Rm[i][j] - Rt[i][j]));
    }
  }
  hold("jacobi3 |S E - E diag|", eig, 1e-14);
  hold("jacobi3 |E^T E - I|", eorth, 1e-14);
  hold("svd3_psd_lapack_signs residual, values", lap, 1e-14);
  hold("svd3 |U S V^T - H|", rec, 1e-14);
  hold("svd3 |U^T U - I|, |V^T V - I|", sorth, 1e-14);
  hold("eigenvalues / singular values descending", order, 0);
  hold("kabsch |det R - 1|", det, 1e-14);
  hold("kabsch planted rotation and translation", rot, 1e-13);
}

static void check_solves() {
  double ne = 0, ax = 0, mn = 0;
  for (int trial = 0; trial < 100; ++trial) {
    R A[36], A0[36], b[6], b0[6], x[6], L[60], rho[6], y[10];
    for (int i = 0; i < 36; ++i) A[i] = A0[i] = uniform();
    for (int i = 0; i < 6; ++i) b[i] = b0[i] = rho[i] = uniform();
    for (int i = 0; i < 60; ++i) L[i] = uniform();
    house_lstsq<6, 3>(A, b, x);                       // the first 18 numbers as a 6 x 3 matrix: A^T (A x - b) = 0
    for (int j = 0; j < 3; ++j) {
      R acc = 0;
      for (int i = 0; i < 6; ++i) acc += A0[i * 3 + j] * (A0[i * 3] * x[0] + A0[i * 3 + 1] * x[1] + A0[i * 3 + 2] * x[2] - b0[i]);
      ne = std::fmax(ne, std::fabs(acc));
    }
    house_minnorm<6, 10>(L, rho, y);                  // L y = rho, and y in the row space of L: y = L^T z for the z of L L^T z = rho
    R G[36], z[6], r2[6];
    for (int i = 0; i < 6; ++i) {
      R acc = -rho[i];
      for (int j = 0; j < 10; ++j) acc += L[i * 10 + j] * y[j];
      ax = std::fmax(ax, std::fabs(acc));
      r2[i] = rho[i];
      for (int k = 0; k < 6; ++k) { G[i * 6 + k] = 0; for (int j = 0; j < 10; ++j) G[i * 6 + k] += L[i * 10 + j] * L[k * 10 + j]; }
    }
    house_lstsq<6, 6>(G, r2, z);
    for (int j = 0; j < 10; ++j) {
      R acc = -y[j];
      for (int i = 0; i < 6; ++i) acc += L[i * 10 + j] * z[i];
      mn = std::fmax(mn, std::fabs(acc));
    }
  }
  hold("house_lstsq |A^T (A x - b)|", ne, 1e-13);
  hold("house_minnorm |L y - rho|", ax, 1e-13);
  hold("house_minnorm |y - L^T (L L^T)^-1 rho|", mn, 1e-10);
}

static void check_epnp() {
  const int sizes[3] = {6, 9, 40};
  double worst[2] = {0, 0};
  for (int trial = 0; trial < 30; ++trial) {
    const int N = sizes[trial % 3];
    std::vector<double> pts(3 * N), pix(2 * N);
    const double K[9] = {500 + 150 * (uniform() + 1), 0, 320, 0, 500 + 150 * (uniform() + 1), 240, 0, 0, 1};
    R Rt[3][3];
    const R tt[3] = {uniform() * 3, uniform() * 3, uniform() * 3};
    random_rotation(Rt);
    for (int n = 0; n < N; ++n) {
      const double z = 6 + 2 * uniform(), c[3] = {0.4 * z * uniform(), 0.4 * z * uniform(), z};
      for (int x = 0; x < 3; ++x) pts[3 * n + x] = Rt[0][x] * (c[0] - tt[0]) + Rt[1][x] * (c[1] - tt[1]) + Rt[2][x] * (c[2] - tt[2]);
      pix[2 * n] = K[0] * c[0] / z + K[2];
      pix[2 * n + 1] = K[4] * c[1] / z + K[5];
    }
    for (int refine = 0; refine < 2; ++refine) {
      SerialContext cx;
      Solver<double, SerialContext> s(cx, pts.data(), pix.data(), K, N);
      R pose[7], Rm[3][3];
      s.solve(refine ? 10 : 0, 1e-28, pose);
      const R x = pose[3], y = pose[4], z = pose[5], w = pose[6];
      const R m[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                         {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                         {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
      for (int i = 0; i < 3; ++i) {
        worst[refine] = std::fmax(worst[refine], std::fabs(pose[i] - tt[i]));
        for (int j = 0; j < 3; ++j) { Rm[i][j] = m[i][j]; worst[refine] = std::fmax(worst[refine], std::fabs(Rm[i][j] - Rt[i][j])); }
      }
      if (!(worst[refine] == worst[refine])) worst[refine] = INFINITY;
    }
  }
  hold("epnp exact data, no refinement: pose error", worst[0], 1e-8);
  hold("epnp exact data, 10 refinement steps: pose error", worst[1], 1e-10);
  // a flat cloud has no third control point: the row is NaN
  SerialContext cx;
  const double flat[18] = {0, 0, 5, 1, 0, 5, 0, 1, 5, 1, 1, 5, 2, 1, 5, -1, 2, 5}, K[9] = {600, 0, 320, 0, 600, 240, 0, 0, 1};
  double pix[12], pose[7];
  for (int n = 0; n < 6; ++n) { pix[2 * n] = 600 * flat[3 * n] / 5 + 320; pix[2 * n + 1] = 600 * flat[3 * n + 1] / 5 + 240; }
  Solver<double, SerialContext> s(cx, flat, pix, K, 6);
  s.solve(10, 1e-28, pose);
  int nans = 0;
  for (int i = 0; i < 7; ++i) nans += pose[i] != pose[i];
  hold("epnp coplanar points: non-NaN entries", 7 - nans, 0);
}

int main() {
  check_jacobi12();
  check_small();
  check_solves();
  check_epnp();
  std::printf(g_failed ? "FAILED\n" : "all identities hold\n");
  return g_failed;
}

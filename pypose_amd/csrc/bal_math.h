// bal_math.h -- per-observation arithmetic of the Snavely / BAL camera model (the reference's examples/module/ba/
// bundle_adjustment.py:16-43, examples/ba.py here) with its closed-form Jacobian blocks.  Host + device like lie_math.h:
// templated on the scalar, compiles with hipcc (csrc/bal.hip) and with g++ (host arithmetic checks).
//
//   q = X . p,  iz = 1 / q_z,  n = -q_xy iz,  rho = n . n,  d = 1 + k1 rho + k2 rho^2
//   r        = f d n - uv
//   dr/df    = d n,   dr/dk1 = f rho n,   dr/dk2 = f rho^2 n
//   A = du/dn = f (d I2 + 2 (k1 + 2 k2 rho) n n^T)                 (2x2, symmetric)
//   dn/dq    = -iz [I2 | n]                                        (2x3)
//   M        = A dn/dq, rows m0, m1
//   dr/dpose  row a = [m_a | q x m_a]     (left tangent, the convention of SE3_Act.backward, as csrc/reproj.hip)
//   dr/dpoint row a = R^T m_a
//
// The division by q_z is the plain division of the model: the BAL model has no homo2cart, so there is no clamp of a depth
// close to zero here (unlike se3_reproj_core).  A zero depth gives a non-finite residual and non-finite pose / point blocks
// in that row and leaves every other row untouched; that is all that is guaranteed.  It is NOT the pattern of the composed
// torch formula: with rho = inf the Horner form below is 1 + inf (k1 + k2 inf) = +-inf where 1 + k1 rho + k2 rho^2 is
// inf - inf = nan for k1, k2 of opposite sign, and the device build's approximate fp64 reciprocal returns nan for 1 / 0
// where IEEE division returns inf (tests/test_bal_host.py, tests/test_bal_edges_gpu.py).
#pragma once
#include "lie_math.h"

namespace pplie {

enum { BAL_JW = 12, BAL_JROW = 2 * BAL_JW };     // one residual row of J: [dK (3) | dpose (6) | dpoint (3)]; J is [n, 2, 12]

// uv == nullptr: zero (r is the projection itself); J == nullptr: residual only
template <class S> PP_HD void se3_bal_core(const S* K, const S* X, const S* p, const S* uv, S* r, S* J) {
  typedef typename Num<S>::base T;
  S qa[3];
  se3_act<S>(X, p, qa);
  const V3<S> q = v3(qa);
  const S iz = S(T(1)) / q.z;
  const S nx = -q.x * iz, ny = -q.y * iz;
  const S rho = nx * nx + ny * ny;
  const S f = K[0], k1 = K[1], k2 = K[2];
  const S d = S(T(1)) + rho * (k1 + k2 * rho);
  const S fd = f * d;
  r[0] = uv ? fd * nx - uv[0] : fd * nx;
  r[1] = uv ? fd * ny - uv[1] : fd * ny;
  if (J) {
    const S frho = f * rho;
    const S c = (S(T(2)) * f) * (k1 + S(T(2)) * k2 * rho);
    const S cx = c * nx, cy = c * ny;
    const S a00 = fd + cx * nx, a01 = cx * ny, a11 = fd + cy * ny;
    const S miz = -iz;
    const V3<S> m0 = v3<S>(miz * a00, miz * a01, miz * (a00 * nx + a01 * ny));
    const V3<S> m1 = v3<S>(miz * a01, miz * a11, miz * (a01 * nx + a11 * ny));
    const V3<S> qv = v3(X + 3);
    const S qw = X[6];
    J[0] = d * nx;
    J[1] = frho * nx;
    J[2] = frho * rho * nx;
    put(m0, J + 3);
    put(cross(q, m0), J + 6);                        // m (-skew(q)) = q x m
    put(adj_rotate_T(qv, qw, m0), J + 9);            // m R = (R^T m)^T
    J[BAL_JW + 0] = d * ny;
    J[BAL_JW + 1] = frho * ny;
    J[BAL_JW + 2] = frho * rho * ny;
    put(m1, J + BAL_JW + 3);
    put(cross(q, m1), J + BAL_JW + 6);
    put(adj_rotate_T(qv, qw, m1), J + BAL_JW + 9);
  }
}

// g J for the three operands at once: gK = g J[:, 0:3], gX = [g J[:, 3:9], 0], gp = g J[:, 9:12]
template <class S> PP_HD void bal_vjp(const S* J, const S* g, S* gK, S* gX, S* gp) {
  typedef typename Num<S>::base T;
#pragma unroll
  for (int c = 0; c < 3; ++c) gK[c] = g[0] * J[c] + g[1] * J[BAL_JW + c];
#pragma unroll
  for (int c = 0; c < 6; ++c) gX[c] = g[0] * J[3 + c] + g[1] * J[BAL_JW + 3 + c];
  gX[6] = S(T(0));
#pragma unroll
  for (int c = 0; c < 3; ++c) gp[c] = g[0] * J[9 + c] + g[1] * J[BAL_JW + 9 + c];
}

}  // namespace pplie

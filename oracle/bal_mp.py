"""ORACLE (test infrastructure only) -- the Snavely / BAL reprojection residual of one observation and its three Jacobian
blocks in 60-digit arithmetic (mpmath).

Conventions are those of pypose_amd/csrc/bal_math.h: ``K = (f, k1, k2)``, ``X = (t, qv, qw)`` (world -> camera),
``q = t + R(qv, qw) p``, ``n = -q_xy / q_z``, ``r = f (1 + k1 |n|^2 + k2 |n|^4) n - uv``; the pose block is the derivative with
respect to a left perturbation ``Exp(delta) * X`` (which the closed form writes ``[m | q x m]``), the point block the
derivative with respect to ``p`` (closed form: ``R^T m``), the intrinsics block with respect to ``K``.

Independent of the code under test on purpose: only the residual is stated here; every Jacobian entry is a central difference
of it at mp precision (step 1e-20: truncation 1e-40, cancellation 1e-40 relative), the pose perturbation through the
exponential map of SE3 (Rodrigues rotation and its left Jacobian), not through any closed-form derivative.

Pure-Python loops: use it for a few hundred rows.
"""
import mpmath as mp
import numpy as np

DPS = 60
H = "1e-20"


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _rotate(qv, qw, p):
    """unit-quaternion rotation p + 2 w (v x p) + 2 v x (v x p)"""
    a = _cross(qv, p)
    b = _cross(qv, a)
    return [p[i] + 2 * qw * a[i] + 2 * b[i] for i in range(3)]


def _se3_exp_act(delta, q):
    """Exp(delta) . q with delta = (tau, phi): R = exp(phi^), translation Jl(phi) tau"""
    tau, phi = delta[:3], delta[3:]
    th2 = phi[0] ** 2 + phi[1] ** 2 + phi[2] ** 2
    if th2 == 0:
        return [q[i] + tau[i] for i in range(3)]
    th = mp.sqrt(th2)
    A, B, C = mp.sin(th) / th, 2 * mp.sin(th / 2) ** 2 / th2, (th - mp.sin(th)) / (th2 * th)
    pq, pt = _cross(phi, q), _cross(phi, tau)
    ppq, ppt = _cross(phi, pq), _cross(phi, pt)
    return [q[i] + A * pq[i] + B * ppq[i] + tau[i] + B * pt[i] + C * ppt[i] for i in range(3)]


def _residual(K, X, p, uv, delta=None):
    q = _rotate(X[3:6], X[6], p)
    q = [q[i] + X[i] for i in range(3)]
    if delta is not None:
        q = _se3_exp_act(delta, q)
    nx, ny = -q[0] / q[2], -q[1] / q[2]
    rho = nx * nx + ny * ny
    s = K[0] * (1 + K[1] * rho + K[2] * rho * rho)
    return [s * nx - uv[0], s * ny - uv[1]]


def bal_mp(K, X, p, uv=None):
    """float64 rows K [n,3], X [n,7], p [n,3], uv [n,2] (None: zero) -> float64 r [n,2], dr/dK [n,2,3], dr/dpose [n,2,6],
    dr/dpoint [n,2,3]; everything in between at DPS digits"""
    n = len(K)
    r, JK, JX, Jp = np.zeros((n, 2)), np.zeros((n, 2, 3)), np.zeros((n, 2, 6)), np.zeros((n, 2, 3))
    with mp.workdps(DPS):
        h = mp.mpf(H)
        for i in range(n):
            Ki, Xi, pi = ([mp.mpf(float(v)) for v in row] for row in (K[i], X[i], p[i]))
            ui = [mp.mpf(0), mp.mpf(0)] if uv is None else [mp.mpf(float(v)) for v in uv[i]]
            r[i] = [float(v) for v in _residual(Ki, Xi, pi, ui)]

            def diff(f, width, out):
                for c in range(width):
                    e = [mp.mpf(0)] * width
                    e[c] = h
                    hi, lo = f(e), f([-v for v in e])
                    out[i, :, c] = [float((a - b) / (2 * h)) for a, b in zip(hi, lo)]

            diff(lambda e: _residual([a + b for a, b in zip(Ki, e)], Xi, pi, ui), 3, JK)
            diff(lambda e: _residual(Ki, Xi, pi, ui, delta=e), 6, JX)
            diff(lambda e: _residual(Ki, Xi, [a + b for a, b in zip(pi, e)], ui), 3, Jp)
    return r, JK, JX, Jp

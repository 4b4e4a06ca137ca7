"""Shared by the tests of the Snavely / BAL reprojection kernels (csrc/bal.hip, csrc/bal_math.h): the formula in plain torch,
the row-relative error, the wide input generator, the fp32 rule for wide inputs and the golden of the reference.  Host only."""
import math
import os

import numpy as np
import torch

F64 = torch.float64
TILE = 128                                              # kBalTile32 = kBalTile64 of csrc/bal.hip: rows per workgroup of lin / vjp
FWD_TILE = 256                                          # kBalFwdTile
GATE = {torch.float32: 1e-5, torch.float64: 2e-9}       # row-relative gates of DESIGN.md section 4
QUANTITIES = ("u", "r", "dK", "dpose", "dpoint")


def load_bal_golden():
    """tests/golden/make_bal_golden.py: K, X, p, uv, r, J_K, J_pose, J_point recorded from the reference in fp64"""
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bal_golden.npz")))


def reference(K, X, p, uv):
    """u, r, dr/dK [n,2,3], dr/dpose [n,2,6], dr/dpoint [n,2,3] by plain torch on the host in the dtype of the inputs, none of
    the package's Lie ops"""
    dt = K.dtype
    t, v, w = X[:, :3], X[:, 3:6], X[:, 6]
    skew = torch.zeros(len(X), 3, 3, dtype=dt)
    skew[:, 0, 1], skew[:, 0, 2], skew[:, 1, 2] = -v[:, 2], v[:, 1], -v[:, 0]
    skew = skew - skew.mT
    R = (1 - 2 * (v * v).sum(-1))[:, None, None] * torch.eye(3, dtype=dt) + 2 * v[:, :, None] * v[:, None, :] + 2 * w[:, None, None] * skew
    q = (t + (R @ p[:, :, None])[:, :, 0]).requires_grad_(True)
    Kg = K.clone().requires_grad_(True)
    n = -q[:, :2] / q[:, 2:]
    rho = (n * n).sum(-1, keepdim=True)
    u = Kg[:, :1] * (1 + Kg[:, 1:2] * rho + Kg[:, 2:3] * rho * rho) * n
    rows = [torch.autograd.grad(u[:, a].sum(), [q, Kg], retain_graph=True) for a in range(2)]
    M, JK = torch.stack([rows[0][0], rows[1][0]], 1), torch.stack([rows[0][1], rows[1][1]], 1)
    qd = q.detach()
    return u.detach(), u.detach() - uv, JK, torch.cat([M, torch.linalg.cross(qd[:, None, :].expand_as(M), M)], -1), M @ R


def row_err(got, want, scale=None):
    """largest absolute error of each row over the row's largest reference magnitude; the worst row"""
    got, want = torch.as_tensor(got).cpu().double().flatten(1), torch.as_tensor(want).double().flatten(1)
    scale = want.abs().amax(-1) if scale is None else scale
    return float(((got - want).abs().amax(-1) / scale).max())


def errors(u, r, J, ref, uv):
    """row_err of the five quantities of a (u [n,2], r [n,2], J [n,24]) result against ``ref = reference(...)`` in fp64"""
    u64, r64, JK, JX, Jp = ref
    Jm = torch.as_tensor(J).reshape(-1, 2, 12)
    return {"u": row_err(u, u64), "r": row_err(r, r64, torch.maximum(u64.abs().amax(-1), uv.double().abs().amax(-1))),
            "dK": row_err(Jm[..., 0:3], JK), "dpose": row_err(Jm[..., 3:9], JX), "dpoint": row_err(Jm[..., 9:12], Jp)}


def wide_inputs(n, dtype, seed=0):
    """K, X, p, uv [n, w] in ``dtype`` on the host, far from a converged problem.  Every row is built from a chosen camera-frame
    point q, p = R^T (q - t), so the conditions hold by construction -- and are asserted on the rounded inputs:
    quaternion half-angle uniform on [0, pi] (rotations up to pi, w of both signs), |t| about 3, |q_z| in [0.5, 20] with both
    signs, |n_x|, |n_y| <= 1.5, f in [200, 2000], |k1| <= 0.3, |k2| <= 0.05, uv about 30 px."""
    g = torch.Generator().manual_seed(seed)
    un = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*(s or (n,)), generator=g, dtype=F64)
    unit = lambda: torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=F64), dim=-1)
    half = un(0.0, math.pi)
    quat = torch.cat([unit() * half.sin()[:, None], half.cos()[:, None]], -1)
    t = unit() * un(2.0, 4.0)[:, None]
    qz = torch.exp(un(math.log(0.501), math.log(19.98))) * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).to(F64)
    q = torch.cat([-un(-1.499, 1.499, n, 2) * qz[:, None], qz[:, None]], -1)
    v, w = quat[:, :3], quat[:, 3:]
    d = q - t
    a = torch.linalg.cross(-v, d)
    p = d + 2 * w * a + 2 * torch.linalg.cross(-v, a)                               # R^T d: rotation by the conjugate
    K = torch.stack([un(200.0, 2000.0), un(-0.3, 0.3), un(-0.05, 0.05)], -1)
    uv = 30 * torch.randn(n, 2, generator=g, dtype=F64)
    K, X, p, uv = [x.to(dtype) for x in (K, torch.cat([t, quat], -1), p, uv)]
    # the conditions, on what the kernels are given
    X64, p64 = X.double(), p.double()
    v, w = X64[:, 3:6], X64[:, 6:]
    a = torch.linalg.cross(v, p64)
    qc = X64[:, :3] + p64 + 2 * w * a + 2 * torch.linalg.cross(v, a)
    nc = -qc[:, :2] / qc[:, 2:]
    assert (w < 0).any() and (w > 0).any() and (qc[:, 2] < 0).any() and (qc[:, 2] > 0).any()
    assert 0.5 <= float(qc[:, 2].abs().min()) and float(qc[:, 2].abs().max()) <= 20 and float(nc.abs().max()) <= 1.5
    assert n < 64 or (float(nc.abs().max()) > 1.3 and float((2 * torch.atan2(v.norm(dim=-1), w[:, 0].abs())).max()) > 3.0)
    return K, X, p, uv


def fp32_rule(errs, ref_errs):
    """The fp32 gate on wide inputs: for each quantity the worst-row error is at most max(1e-5, 4 x E_ref), E_ref the worst-row
    error of the plain fp32 torch formula on the same rows.  The fixed 1e-5 cannot be kept there: the formula itself, in fp32
    against fp64 on the same fp32-rounded inputs, is up to 4.9e-4 off in u (cancellation in t + R p, rows with small |n|).  The
    margin 4: the kernel rotates by quaternion where the formula multiplies by a matrix, which reorders the rounding of R p
    but does not change its magnitude.  Returns {quantity: (error, bound, error / E_ref)}."""
    out = {k: (errs[k], max(GATE[torch.float32], 4 * ref_errs[k]), errs[k] / ref_errs[k]) for k in errs}
    return out, all(e <= b for e, b, _ in out.values())


def formula_errors(host):
    """E_ref of fp32_rule: reference() run in the dtype of ``host`` = (K, X, p, uv) against reference() in fp64 on the same
    rounded inputs; also returns the fp64 reference"""
    ref = reference(*[t.double() for t in host])
    u, r, JK, JX, Jp = reference(*host)
    return errors(u, r, torch.cat([JK, JX, Jp], -1), ref, host[3]), ref

"""Golden residuals and Jacobian blocks of the Snavely / BAL reprojection model from the REAL reference:
    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python tests/golden/make_bal_golden.py

The model is the one make_ba_golden.py states (the reference example's Reproj.project minus the observation); the values come
from the reference's own SE3.Act and autograd in fp64, one observation per row:
  r [n,2], J_K = dr/dK [n,2,3], J_pose = dr/dpose [n,2,6] (the first six components of the gradient on an SE3 parameter: left
  tangent; the seventh is asserted zero), J_point = dr/dpoint [n,2,3].
Inputs on purpose far from the gentle ones of a converged problem: the quaternion half-angle covers [0, pi] (rotations up to
pi, w of both signs), points in front of and behind the camera, |n| up to 1.5 per axis, k1 / k2 of both signs, f in
[200, 2000].  Each row is built from its camera-frame point q: p = R^T (q - t)."""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
import pypose as pp  # noqa: E402  the reference

D = torch.float64
n = 48
g = torch.Generator().manual_seed(11)
un = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*(s or (n,)), generator=g, dtype=D)
half = un(0.0, np.pi)
half[0], half[1], half[2], half[3] = np.pi / 2, np.pi / 2 + 1e-9, np.pi, 0.0    # rotation by pi (w = 0), just past it, w = -1, w = 1
axis = torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=D), dim=-1)
quat = torch.cat([axis * half.sin()[:, None], half.cos()[:, None]], -1)
quat[0, 3] = 0.0
quat = torch.nn.functional.normalize(quat, dim=-1)
t = torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=D), dim=-1) * un(2.0, 4.0)[:, None]
X = pp.SE3(torch.cat([t, quat], -1))
qz = torch.exp(un(np.log(0.5), np.log(20.0))) * torch.where(torch.arange(n) % 3 == 1, -1.0, 1.0).to(D)   # a third behind the camera
nxy = un(-1.5, 1.5, n, 2)
nxy[4], nxy[5], nxy[6] = torch.tensor([1.5, -1.5], dtype=D), torch.tensor([0.0, 1e-3], dtype=D), torch.tensor([1e-4, 0.0], dtype=D)
q = torch.cat([-nxy * qz[:, None], qz[:, None]], -1)
p = X.Inv().Act(q)
sign = lambda k: torch.where((torch.arange(n) // k) % 2 == 0, 1.0, -1.0).to(D)
K = torch.stack([un(200.0, 2000.0), sign(1) * un(0.0, 0.3), sign(2) * un(0.0, 0.05)], -1)     # all four sign pairs of (k1, k2)
K[0, 0], K[1, 0] = 200.0, 2000.0
uv = 30 * torch.randn(n, 2, generator=g, dtype=D)
assert float((quat[:, 3] < 0).sum()) >= 10 and float((quat[:, 3] > 0).sum()) >= 10


def project(K, C, P):           # examples/module/ba/bundle_adjustment.py:16-43, as make_ba_golden.py
    cp = C.Act(P)
    nn = - cp[..., :2] / cp[..., [2]]
    radius = nn.square().sum(dim=-1, keepdim=True)
    focal, k1, k2 = K[..., :1], K[..., 1:2], K[..., 2:3]
    distortion = 1 + k1 * radius + k2 * radius.square()
    return focal * distortion * nn


Kr, Xp, pr = K.clone().requires_grad_(True), pp.Parameter(X.clone()), p.clone().requires_grad_(True)
r = project(Kr, Xp, pr) - uv
JK, JX, Jp = [], [], []
for a in range(2):
    gK, gX, gP = torch.autograd.grad(r[:, a].sum(), [Kr, Xp, pr], retain_graph=True)
    assert float(gX[:, 6].abs().max()) == 0
    JK.append(gK), JX.append(gX[:, :6]), Jp.append(gP)
S = {"K": K, "X": X.tensor(), "p": p, "uv": uv, "r": r, "J_K": torch.stack(JK, 1), "J_pose": torch.stack(JX, 1),
     "J_point": torch.stack(Jp, 1)}
cam = Xp.detach().Act(p)
nrm = -cam[:, :2] / cam[:, 2:]
print("rows", n, "w<0", int((quat[:, 3] < 0).sum()), "behind", int((cam[:, 2] < 0).sum()), "max|n_axis|", float(nrm.abs().max()),
      "max rotation", float((2 * torch.atan2(quat[:, :3].norm(dim=-1), quat[:, 3].abs())).max()), "max|r|", float(r.detach().abs().max()))
np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "bal_golden.npz"),
                    **{k: v.detach().numpy() for k, v in S.items()})
print("ok", len(S))

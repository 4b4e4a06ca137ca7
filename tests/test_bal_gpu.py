"""Closed-form Snavely / BAL reprojection on the MI355X (csrc/bal.hip, function/geometry.py bal_reprojerr): the three kernels
against the formula in plain fp64 torch, the autograd wiring against the hand-written model of examples/ba.py, and LM taking
the closed-form blocks of all three parameters."""
import pytest
import torch

import pypose_amd as pp
from pypose_amd.function import geometry as geo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = 128                                              # kBalTile32 of csrc/bal.hip: rows per workgroup of lin / vjp in fp32
GATE = {torch.float32: 1e-5, torch.float64: 2e-9}       # row-relative gates of DESIGN.md section 4
F64 = torch.float64


def inputs(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    un = lambda lo, hi: lo + (hi - lo) * torch.rand(n, generator=g, dtype=F64)
    X = pp.se3((0.1 * rn(n, 6)).to(DEV)).Exp().tensor().cpu()
    p = rn(n, 3) + torch.tensor([0.0, 0.0, 6.0], dtype=F64)
    K = torch.stack([un(400, 600), un(-0.1, 0.1), un(-0.01, 0.01)], -1)
    return K, X, p, 3 * rn(n, 2)


def reference(K, X, p, uv):
    """u, r, dr/dK [n,2,3], dr/dpose [n,2,6], dr/dpoint [n,2,3] in fp64 torch on the host, none of the package's Lie ops"""
    t, v, w = X[:, :3], X[:, 3:6], X[:, 6]
    skew = torch.zeros(len(X), 3, 3, dtype=F64)
    skew[:, 0, 1], skew[:, 0, 2], skew[:, 1, 2] = -v[:, 2], v[:, 1], -v[:, 0]
    skew = skew - skew.mT
    R = (1 - 2 * (v * v).sum(-1))[:, None, None] * torch.eye(3, dtype=F64) + 2 * v[:, :, None] * v[:, None, :] + 2 * w[:, None, None] * skew
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
    got, want = got.cpu().double().flatten(1), want.flatten(1)
    scale = want.abs().amax(-1) if scale is None else scale
    return float(((got - want).abs().amax(-1) / scale).max())


@pytest.mark.parametrize("n", [1, 63, TILE + 1, 2 * TILE + 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_kernels_match_fp64_formula(dtype, n):
    host = [t.to(dtype) for t in inputs(n)]
    u, r_ref, JK, JX, Jp = reference(*[t.double() for t in host])
    K, X, p, uv = [t.to(DEV) for t in host]
    r, J = geo._bal_lin(K, X, p, uv)
    assert torch.equal(geo._bal_fwd(K, X, p, uv), r)
    Jm = J.view(n, 2, 12)
    errs = {"r": row_err(r, r_ref, torch.maximum(u.abs().amax(-1), host[3].double().abs().amax(-1))),
            "u": row_err(geo._bal_fwd(K, X, p), u),                     # a null uv: the projection itself
            "dK": row_err(Jm[..., 0:3], JK), "dpose": row_err(Jm[..., 3:9], JX), "dpoint": row_err(Jm[..., 9:12], Jp)}
    g = torch.randn(n, 2, dtype=F64, generator=torch.Generator().manual_seed(1)).to(dtype)
    gK, gX, gp = geo._bal_vjp(J, g.to(DEV))
    want = torch.einsum("na,nac->nc", g.double(), Jm.cpu().double())
    errs.update(gK=row_err(gK, want[:, 0:3]), gX=row_err(gX[:, :6], want[:, 3:9]), gp=row_err(gp, want[:, 9:12]))
    print(dtype, n, {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v <= GATE[dtype] for v in errs.values()), errs
    assert float(gX[:, 6].abs().max()) == 0


def ba_formula(K, C, P):
    """the hand-written projection of examples/ba.py"""
    cp = C.Act(P)
    n = - cp[..., :2] / cp[..., [2]]
    radius = n.square().sum(dim=-1, keepdim=True)
    return K[..., :1] * (1 + K[..., 1:2] * radius + K[..., 2:3] * radius.square()) * n


@pytest.mark.parametrize("shared_K", [False, True])
def test_autograd_matches_composed_model(shared_K):
    K, X, p, uv = [t.to(DEV) for t in inputs(130, seed=2)]
    K = K[:1] if shared_K else K                       # one row of intrinsics for every observation: sum_to_size
    w = torch.randn(130, 2, dtype=F64, generator=torch.Generator().manual_seed(3)).to(DEV)
    got = []
    for model in (lambda K, C, P: pp.bal_reprojerr(P, uv, K, C), lambda K, C, P: ba_formula(K, C, P) - uv):
        leaves = [K.clone().requires_grad_(True), pp.Parameter(pp.SE3(X.clone())), p.clone().requires_grad_(True)]
        r = model(*leaves)
        got.append([r.detach(), *torch.autograd.grad((r * w).sum(), leaves)])
    for a, b in zip(*got):
        torch.testing.assert_close(torch.Tensor.as_subclass(a, torch.Tensor), torch.Tensor.as_subclass(b, torch.Tensor),
                                   rtol=1e-9, atol=1e-9)


class BA(torch.nn.Module):
    def __init__(self, K, C, P, closed):
        super().__init__()
        self.K, self.C, self.P = pp.Parameter(K, sjac=True), pp.Parameter(C, sjac=True), pp.Parameter(P, sjac=True)
        self.closed = closed

    def forward(self, observe, cidx, pidx):
        if self.closed:
            return pp.bal_reprojerr(self.P[pidx], observe, self.K[cidx], self.C[cidx])
        return ba_formula(self.K[cidx], self.C[cidx], self.P[pidx]) - observe


def test_lm_takes_closed_form_blocks():
    Nc, Np = 4, 24
    K, X, _, _ = inputs(Nc, seed=4)
    P = inputs(Np, seed=5)[2]
    g = torch.Generator().manual_seed(6)
    cidx, pidx = torch.arange(Nc).repeat_interleave(Np).to(DEV), torch.arange(Np).repeat(Nc).to(DEV)
    K, P, C = K.to(DEV), P.to(DEV), pp.SE3(X.to(DEV))
    observe = ba_formula(K[cidx], C[cidx], P[pidx])
    C0 = pp.se3((0.02 * torch.randn(Nc, 6, dtype=F64, generator=g)).to(DEV)).Exp() @ C
    P0 = P + (0.05 * torch.randn(Np, 3, dtype=F64, generator=g)).to(DEV)
    runs = {}
    for closed in (True, False):
        model = BA(K.clone(), pp.SE3(C0.tensor().clone()), P0.clone(), closed).to(DEV)
        opt = pp.optim.LM(model, strategy=pp.optim.strategy.TrustRegion(radius=1e4), min=1e-6)
        runs[closed] = [float(opt.step((observe, cidx, pidx))) for _ in range(4)]
        assert opt.linearization == "multigraph" and opt._last_blocks == ("closed-form" if closed else "autograd")
    print(runs)
    torch.testing.assert_close(torch.tensor(runs[True], dtype=F64), torch.tensor(runs[False], dtype=F64), rtol=1e-8, atol=0)
    assert runs[True][-1] < runs[True][0]

"""Closed-form Snavely / BAL reprojection on the MI355X (csrc/bal.hip, function/geometry.py bal_reprojerr): the three kernels
against the formula in plain fp64 torch, the autograd wiring against the hand-written model of examples/ba.py, and LM taking
the closed-form blocks of all three parameters."""
import numpy as np
import pytest
import torch

import pypose_amd as pp
from pypose_amd.function import geometry as geo
from tests.bal_util import (F64, FWD_TILE, GATE, TILE, errors, formula_errors, fp32_rule, load_bal_golden, reference, row_err,
                            wide_inputs)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
plain = lambda t: torch.Tensor.as_subclass(t, torch.Tensor)


def inputs(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    un = lambda lo, hi: lo + (hi - lo) * torch.rand(n, generator=g, dtype=F64)
    X = pp.se3((0.1 * rn(n, 6)).to(DEV)).Exp().tensor().cpu()
    p = rn(n, 3) + torch.tensor([0.0, 0.0, 6.0], dtype=F64)
    K = torch.stack([un(400, 600), un(-0.1, 0.1), un(-0.01, 0.01)], -1)
    return K, X, p, 3 * rn(n, 2)


@pytest.mark.parametrize("n", [1, 3, 4, 63, TILE - 1, TILE, TILE + 1, FWD_TILE - 1, 2 * TILE, FWD_TILE + 1, 2 * TILE + 3])
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
    # g J is a sum of two products per entry.  All three entries of a gK row carry the factor g . n, so a row whose two terms
    # cancel (n = 257 has one, 300-fold) is small against its terms in every entry and no arithmetic of the format keeps
    # 1e-5 of the row's largest result there.  The scale of a row is therefore that of its terms, |g| |J|, and each entry
    # also holds the rounding bound of a two-term dot product, 2 eps of its own terms -- far tighter than the gate.
    terms = torch.einsum("na,nac->nc", g.double().abs(), Jm.cpu().double().abs())
    got = torch.cat([gK.cpu(), gX[:, :6].cpu(), gp.cpu()], -1).double()
    for k, sl in (("gK", slice(0, 3)), ("gX", slice(3, 9)), ("gp", slice(9, 12))):
        errs[k] = row_err(got[:, sl], want[:, sl], terms[:, sl].amax(-1))
    print(dtype, n, {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v <= GATE[dtype] for v in errs.values()), errs
    assert bool(((got - want).abs() <= 2 * torch.finfo(dtype).eps * terms).all())
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


# ---- wide inputs: rotations up to pi, negative w, points behind the camera, |n| up to 1.5 per axis, rho of order 1

def kernel_results(host):
    K, X, p, uv = [t.to(DEV) for t in host]
    r, J = geo._bal_lin(K, X, p, uv)
    assert torch.equal(geo._bal_fwd(K, X, p, uv), r)
    return geo._bal_fwd(K, X, p), r, J


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_kernels_on_wide_inputs(dtype):
    """fp64: the 2e-9 gate.  fp32: the fixed 1e-5 cannot hold here -- the plain torch formula in fp32 is itself up to 4.9e-4
    off in u on such rows (cancellation in t + R p, small |n|) -- so each quantity is held to max(1e-5, 4 x E_ref), E_ref the
    worst-row error of reference() in fp32 on the same rows (tests/bal_util.py fp32_rule).
    Measured on the MI355X (n = 259, seed 0), kernel error (ratio to E_ref): u 1.17e-5 (2.21), r 1.17e-5 (2.23), dK 2.62e-6
    (0.95), dpose 4.03e-6 (1.79), dpoint 4.03e-6 (1.66); fp64 at most 1.5e-14."""
    host = wide_inputs(2 * TILE + 3, dtype)
    ref_errs, ref = formula_errors(host)
    errs = errors(*kernel_results(host), ref, host[3])
    if dtype == F64:
        print(dtype, {k: f"{v:.2e}" for k, v in errs.items()})
        assert all(v <= GATE[F64] for v in errs.values()), errs
    else:
        out, ok = fp32_rule(errs, ref_errs)
        print(dtype, {k: f"{e:.2e} (bound {b:.2e}, x{q:.2f} of the formula)" for k, (e, b, q) in out.items()})
        assert ok, out


def test_kernels_reproduce_the_reference_golden():
    """the reference's own SE3.Act and autograd, recorded in fp64 (tests/golden/make_bal_golden.py)"""
    G = {k: torch.from_numpy(v) for k, v in load_bal_golden().items()}
    gold = (G["r"] + G["uv"], G["r"], G["J_K"], G["J_pose"], G["J_point"])
    errs = errors(*kernel_results([G[k] for k in ("K", "X", "p", "uv")]), gold, G["uv"])
    print({k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v <= GATE[F64] for v in errs.values()), errs


# ---- the autograd wrapper: shapes, strides, dtypes, routes

def grads_of(model, leaves, w):
    r = model(*leaves)
    return [r.detach(), *[plain(g) for g in torch.autograd.grad((r * w).sum(), leaves)]]


def close64(a, b):
    torch.testing.assert_close(plain(a), plain(b), rtol=1e-9, atol=1e-9)


def batched_leaves(B, N, K_lead, dtype=F64, seed=10):
    K, X, p, uv = inputs(B * N, seed=seed)
    K = K[:K_lead].reshape(K_lead, 1, 3)
    return [K.to(dtype).to(DEV).requires_grad_(True), pp.Parameter(pp.SE3(X[:B].reshape(B, 1, 7).to(dtype).to(DEV))),
            p.reshape(B, N, 3).to(dtype).to(DEV).requires_grad_(True)], uv.reshape(B, N, 2).to(dtype).to(DEV)


@pytest.mark.parametrize("K_lead", [1, 3])
def test_batched_shapes_broadcast(K_lead):
    """points [B,N,3] against poses [B,1,7] and K [1,1,3] / [B,1,3], pixels [B,N,2]: gradients in each leaf's own shape"""
    B, N = 3, 50
    leaves, uv = batched_leaves(B, N, K_lead)
    w = torch.randn(B, N, 2, dtype=F64, generator=torch.Generator().manual_seed(11)).to(DEV)
    got = grads_of(lambda K, C, P: pp.bal_reprojerr(P, uv, K, C), leaves, w)
    want = grads_of(lambda K, C, P: ba_formula(K, C, P) - uv, leaves, w)
    assert got[0].shape == (B, N, 2) and [tuple(g.shape) for g in got[1:]] == [(K_lead, 1, 3), (B, 1, 7), (B, N, 3)]
    for a, b in zip(got, want):
        close64(a, b)


def test_strided_and_expanded_operands():
    """a transposed-then-sliced points tensor and an expanded pose: values and gradients are those of the contiguous copies,
    bit for bit"""
    N = 131
    K, X, p, uv = [t.to(DEV) for t in inputs(N + 4, seed=12)]
    K, uv = K[:N], uv[:N]
    base = p.T.contiguous().requires_grad_(True)                   # [3, N + 4]
    pose = X[:1].clone().requires_grad_(True)                      # [1, 7]
    w = torch.randn(N, 2, dtype=F64, generator=torch.Generator().manual_seed(13)).to(DEV)
    out = []
    for copy in (False, True):
        pts, Xe = base.T[2:-2], pose.expand(N, 7)
        assert not pts.is_contiguous() and not Xe.is_contiguous()
        if copy:
            pts, Xe = pts.contiguous(), Xe.contiguous()
        r = pp.bal_reprojerr(pts, uv, K, pp.SE3(Xe))
        out.append([r.detach(), *torch.autograd.grad((r * w).sum(), [base, pose])])
    for a, b in zip(*out):
        assert torch.equal(plain(a), plain(b))
    assert float(out[0][2][:, 6].abs().max()) == 0 and float(out[0][1][:, :2].abs().max()) == 0


def fp32_checked(got, want64, composed32, names):
    """the fp32 rule of test_kernels_on_wide_inputs with the composed fp32 result as E_ref, per returned tensor"""
    errs = {k: row_err(plain(a).reshape(-1, a.shape[-1]), plain(b).cpu().reshape(-1, b.shape[-1])) for k, a, b in zip(names, got, want64)}
    refs = {k: row_err(plain(a).reshape(-1, a.shape[-1]), plain(b).cpu().reshape(-1, b.shape[-1])) for k, a, b in zip(names, composed32, want64)}
    out, ok = fp32_rule(errs, {k: max(v, 1e-30) for k, v in refs.items()})
    print({k: f"{e:.2e} (bound {b:.2e})" for k, (e, b, _) in out.items()})
    assert ok, out


def test_fp32_forward_and_backward():
    N = 2 * TILE + 3
    K, X, p, uv = [t.float().to(DEV) for t in inputs(N, seed=14)]
    w = torch.randn(N, 2, generator=torch.Generator().manual_seed(15)).to(DEV)
    leaves = lambda dt: [K.to(dt).requires_grad_(True), pp.Parameter(pp.SE3(X.to(dt))), p.to(dt).requires_grad_(True)]
    got = grads_of(lambda K, C, P: pp.bal_reprojerr(P, uv, K, C), leaves(torch.float32), w)
    comp = grads_of(lambda K, C, P: ba_formula(K, C, P) - uv, leaves(torch.float32), w)
    want = grads_of(lambda K, C, P: ba_formula(K, C, P) - uv.double(), leaves(F64), w.double())
    assert all(t.dtype == torch.float32 for t in got)
    got[2], comp[2], want[2] = got[2][:, :6], comp[2][:, :6], want[2][:, :6]
    # r is small next to u and uv on some rows: its error is measured against the projection, as in the kernel tests
    u64 = want[0] + uv.double()
    scale = torch.maximum(u64.abs().amax(-1), uv.double().abs().amax(-1)).cpu()
    e_r, e_ref = row_err(got[0], want[0].cpu(), scale), row_err(comp[0], want[0].cpu(), scale)
    assert e_r <= max(1e-5, 4 * e_ref), (e_r, e_ref)
    fp32_checked(got[1:], want[1:], comp[1:], ("gK", "gX", "gp"))


@pytest.mark.parametrize("broadcast", [False, True])
def test_gradient_of_pixels(broadcast):
    N = 130
    K, X, p, uv = [t.to(DEV) for t in inputs(N, seed=16)]
    uv = (uv[:1] if broadcast else uv).clone().requires_grad_(True)
    P = p.clone().requires_grad_(True)
    w = torch.randn(N, 2, dtype=F64, generator=torch.Generator().manual_seed(17)).to(DEV)
    r = pp.bal_reprojerr(P, uv, K, pp.SE3(X))
    g_uv, g_p = torch.autograd.grad((r * w).sum(), [uv, P])
    assert g_uv.shape == uv.shape
    if broadcast:
        torch.testing.assert_close(g_uv, -w.sum(0, keepdim=True), rtol=1e-12, atol=1e-12)
    else:
        assert torch.equal(g_uv, -w)
    Pc = p.clone().requires_grad_(True)
    close64(g_p, torch.autograd.grad(((ba_formula(K, pp.SE3(X), Pc) - uv.detach()) * w).sum(), [Pc])[0])


@pytest.mark.parametrize("reduction", ["norm", "sum"])
def test_reductions(reduction):
    N = 130
    K, X, p, uv = [t.to(DEV) for t in inputs(N, seed=18)]
    w = torch.randn(N, dtype=F64, generator=torch.Generator().manual_seed(19)).to(DEV)
    red = {"norm": lambda e: e.norm(dim=-1), "sum": lambda e: e.sum(dim=-1)}[reduction]
    leaves = lambda: [K.clone().requires_grad_(True), pp.Parameter(pp.SE3(X.clone())), p.clone().requires_grad_(True)]
    got = grads_of(lambda K, C, P: pp.bal_reprojerr(P, uv, K, C, reduction=reduction), leaves(), w)
    want = grads_of(lambda K, C, P: red(ba_formula(K, C, P) - uv), leaves(), w)
    assert got[0].shape == (N,)
    for a, b in zip(got, want):
        close64(a, b)


@pytest.mark.parametrize("dtype", [torch.float32, F64])
def test_point2pixel_with_and_without_gradients(dtype):
    """gradients required: the lin kernel with a NULL uv; without: the fwd kernel, the same bits"""
    N = 2 * TILE + 3
    K, X, p, _ = [t.to(dtype).to(DEV) for t in inputs(N, seed=20)]
    w = torch.randn(N, 2, dtype=F64, generator=torch.Generator().manual_seed(21)).to(dtype).to(DEV)
    leaves = lambda dt: [K.to(dt).requires_grad_(True), pp.Parameter(pp.SE3(X.to(dt))), p.to(dt).requires_grad_(True)]
    got = grads_of(lambda K, C, P: pp.bal_point2pixel(P, K, C), leaves(dtype), w)
    with torch.no_grad():
        assert torch.equal(pp.bal_point2pixel(p, K, pp.SE3(X)), got[0])
    assert torch.equal(geo._bal_fwd(K, X, p), got[0]) and torch.equal(geo._bal_lin(K, X, p)[0], got[0])
    want = grads_of(ba_formula, leaves(F64), w.double())
    if dtype == F64:
        for a, b in zip(got, want):
            close64(a, b)
    else:
        comp = grads_of(ba_formula, leaves(dtype), w)
        for t in (got, comp, want):
            t[2] = t[2][:, :6]
        fp32_checked(got, want, comp, ("u", "gK", "gX", "gp"))


def test_second_order_route():
    """create_graph=True: the backward is recorded from differentiable ops; a Hessian-vector product equals ba_formula's"""
    N = 40
    K, X, p, uv = [t.to(DEV) for t in inputs(N, seed=22)]
    g = torch.Generator().manual_seed(23)
    w = torch.randn(N, 2, dtype=F64, generator=g).to(DEV)
    vs = [torch.randn(N, k, dtype=F64, generator=g).to(DEV) for k in (3, 7, 3)]
    out = []
    for model in (lambda K, C, P: pp.bal_reprojerr(P, uv, K, C), lambda K, C, P: ba_formula(K, C, P) - uv):
        leaves = [K.clone().requires_grad_(True), pp.Parameter(pp.SE3(X.clone())), p.clone().requires_grad_(True)]
        r = model(*leaves)
        first = torch.autograd.grad((r * w).sum() + (r * r).sum(), leaves, create_graph=True)
        out.append(torch.autograd.grad(sum((plain(a) * v).sum() for a, v in zip(first, vs)), leaves))
    for a, b in zip(*out):
        torch.testing.assert_close(plain(a), plain(b), rtol=1e-8, atol=1e-8)


def test_vectorised_routes():
    N = 37
    K, X, p, uv = [t.to(DEV) for t in inputs(N, seed=24)]
    C = pp.SE3(X)
    Jv = torch.autograd.functional.jacobian(lambda P: pp.bal_reprojerr(P, uv, K, C), p, vectorize=True)        # [N,2,N,3]
    Jp = geo._bal_lin(K, X, p, uv)[1].view(N, 2, 12)[..., 9:12]
    idx = torch.arange(N, device=DEV)
    close64(Jv[idx, :, idx], Jp)
    off = Jv.clone()
    off[idx, :, idx] = 0
    assert float(off.abs().max()) == 0
    # torch.func.vmap over a leading dimension of the points equals the loop
    B = 3
    Pb = torch.stack([p + 0.01 * k for k in range(B)])
    got = torch.func.vmap(lambda P: pp.bal_reprojerr(P, uv, K, C))(Pb)
    close64(got, torch.stack([pp.bal_reprojerr(Pb[k], uv, K, C) for k in range(B)]))


def test_fall_backs_take_the_composed_route(monkeypatch):
    N = 33
    K, X, p, uv = inputs(N, seed=25)
    calls = []
    real = geo._bal_call
    monkeypatch.setattr(geo, "_bal_call", lambda *a, **k: (calls.append(a[0]), real(*a, **k))[1])
    want = ba_formula(K.to(DEV), pp.SE3(X.to(DEV)), p.to(DEV)) - uv.to(DEV)
    # host tensors
    r = pp.bal_reprojerr(p, uv, K, pp.SE3(X))
    assert not r.is_cuda and not calls
    close64(r, want.cpu())
    # mixed dtypes of K and points: type promotion of the composed model
    r = pp.bal_reprojerr(p.to(DEV), uv.to(DEV), K.float().to(DEV), pp.SE3(X.to(DEV)))
    assert r.dtype == F64 and not calls
    close64(r, ba_formula(K.float().to(DEV), pp.SE3(X.to(DEV)), p.to(DEV)) - uv.to(DEV))
    # half precision does not reach the kernels
    try:
        pp.bal_reprojerr(p.half().to(DEV), uv.half().to(DEV), K.half().to(DEV), pp.SE3(X.half().to(DEV)))
    except (RuntimeError, TypeError):
        pass                                               # (the Lie ops have no half kernels either: an error, not a launch)
    assert not calls
    pp.bal_reprojerr(p.to(DEV), uv.to(DEV), K.to(DEV), pp.SE3(X.to(DEV)))
    assert calls == ["se3_bal_fwd"]


# ---- LM on the closed-form blocks in fp32, with a robust kernel, and on the reference's recorded trajectory

def lm_runs(dtype, steps=4, **lm_kw):
    """test_lm_takes_closed_form_blocks in another dtype / with a robust kernel.  The observations carry 0.5 px of noise: with
    exact observations the loss falls to the rounding floor of fp32 within the four steps, where two routes that differ in
    the last bits have no relative agreement to speak of"""
    Nc, Np = 4, 24
    K, X, _, _ = inputs(Nc, seed=4)
    P = inputs(Np, seed=5)[2]
    g = torch.Generator().manual_seed(6)
    cidx, pidx = torch.arange(Nc).repeat_interleave(Np).to(DEV), torch.arange(Np).repeat(Nc).to(DEV)
    K, P, C = K.to(DEV), P.to(DEV), pp.SE3(X.to(DEV))
    observe = ba_formula(K[cidx], C[cidx], P[pidx]) + 0.5 * torch.randn(Nc * Np, 2, dtype=F64, generator=g).to(DEV)
    C0 = pp.se3((0.02 * torch.randn(Nc, 6, dtype=F64, generator=g)).to(DEV)).Exp() @ C
    P0 = P + (0.05 * torch.randn(Np, 3, dtype=F64, generator=g)).to(DEV)
    runs = {}
    for closed in (True, False):
        model = BA(K.to(dtype).clone(), pp.SE3(C0.tensor().to(dtype).clone()), P0.to(dtype).clone(), closed).to(DEV)
        opt = pp.optim.LM(model, strategy=pp.optim.strategy.TrustRegion(radius=1e4), min=1e-6, **lm_kw)
        runs[closed] = [float(opt.step((observe.to(dtype), cidx, pidx))) for _ in range(steps)]
        assert opt.linearization == "multigraph" and opt._last_blocks == ("closed-form" if closed else "autograd")
    print(runs)
    return runs


def test_lm_takes_closed_form_blocks_fp32():
    runs = lm_runs(torch.float32)
    torch.testing.assert_close(torch.tensor(runs[True], dtype=F64), torch.tensor(runs[False], dtype=F64), rtol=1e-4, atol=0)
    assert runs[True][-1] < runs[True][0]


def test_lm_takes_closed_form_blocks_with_a_huber_kernel():
    runs = lm_runs(F64, kernel=pp.optim.kernel.Huber(delta=1.0))
    torch.testing.assert_close(torch.tensor(runs[True], dtype=F64), torch.tensor(runs[False], dtype=F64), rtol=1e-8, atol=0)
    assert runs[True][-1] < runs[True][0]


def test_closed_form_route_replays_the_reference_trajectory():
    """ba_golden.npz's ba_small (the reference's dense LM on the same model): the tolerances of tests/test_ba_gpu.py"""
    from tests.optim_models import T, compare_trajectory, load_ba_golden, run_steps
    G = load_ba_golden()
    tag = "ba_small"
    model = BA(T(G[f"{tag}/K0"], DEV), pp.SE3(T(G[f"{tag}/C0"], DEV)), T(G[f"{tag}/P0"], DEV), True)
    opt = pp.optim.LM(model, solver=pp.optim.solver.Cholesky(), strategy=pp.optim.strategy.TrustRegion(radius=1e4), min=1e-6)
    opt.structured = True
    args = (T(G[f"{tag}/obs"], DEV), T(G[f"{tag}/cidx"], DEV), T(G[f"{tag}/pidx"], DEV))
    rec = run_steps(opt, (args,), {}, 6)
    assert set(rec["kind"]) == {"multigraph"} and opt._last_blocks == "closed-form"
    compare_trajectory(rec, G, tag, floor=1e-12, rtol=1e-7)
    np.testing.assert_allclose(model.P.detach().cpu().numpy(), G[f"{tag}/P"], atol=1e-6)
    np.testing.assert_allclose(model.C.detach().tensor().cpu().numpy(), G[f"{tag}/C"], atol=1e-6)

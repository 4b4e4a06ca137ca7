"""The arithmetic of the Snavely / BAL reprojection kernels (csrc/bal_math.h) without a GPU, anchored three ways: the golden
recorded from the reference's own SE3.Act and autograd (tests/golden/make_bal_golden.py), a 60-digit oracle whose Jacobians are
central differences of the residual (oracle/bal_mp.py), and bal_math.h itself compiled with g++ (tests/hostmath).  The inputs
are wide on purpose: rotations up to pi, negative w, points behind the camera, |n| up to 1.5 per axis."""
import numpy as np
import pytest
import torch

import pypose_amd as pp
from oracle.bal_mp import bal_mp
from tests.bal_util import (F64, GATE, TILE, errors, formula_errors, fp32_rule, load_bal_golden, reference, row_err,
                            wide_inputs)
from tests.hostmath_util import hostmath_bal_core, hostmath_bal_vjp
from tests.oracle_backend import oracle_backend


@pytest.fixture(scope="module")
def G():
    return load_bal_golden()


@pytest.fixture(scope="module")
def gold(G):
    """the golden as reference()'s tuple: u, r, dK, dpose, dpoint in fp64"""
    t = {k: torch.from_numpy(v) for k, v in G.items()}
    return t["r"] + t["uv"], t["r"], t["J_K"], t["J_pose"], t["J_point"]


@pytest.fixture(scope="module")
def mp_blocks(G):
    return bal_mp(G["K"], G["X"], G["p"], G["uv"])


def golden_inputs(G, dtype=F64):
    return [torch.from_numpy(G[k]).to(dtype) for k in ("K", "X", "p", "uv")]


def test_golden_covers_the_wide_ranges(G):
    K, X, p, uv = golden_inputs(G)
    assert len(K) == 48 and G["J_K"].shape == (48, 2, 3) and G["J_pose"].shape == (48, 2, 6) and G["J_point"].shape == (48, 2, 3)
    w = X[:, 6]
    v = X[:, 3:6]
    a = torch.linalg.cross(v, p)
    q = X[:, :3] + p + 2 * w[:, None] * a + 2 * torch.linalg.cross(v, a)
    nrm = -q[:, :2] / q[:, 2:]
    assert (w < 0).sum() >= 10 and (w > 0).sum() >= 10 and float(w.abs().min()) == 0            # a rotation by exactly pi
    assert (q[:, 2] < 0).sum() >= 10 and (q[:, 2] > 0).sum() >= 10
    assert 1.49 < float(nrm.abs().max()) <= 1.5 + 1e-12
    assert float(K[:, 0].min()) == 200 and float(K[:, 0].max()) == 2000
    assert {(bool(a), bool(b)) for a, b in (K[:, 1:] > 0).tolist()} == {(False, False), (False, True), (True, False), (True, True)}


def test_mp_oracle_agrees_with_the_reference_golden(G, gold, mp_blocks):
    r, JK, JX, Jp = mp_blocks
    errs = errors(gold[0], r, np.concatenate([JK, JX, Jp], -1), gold, torch.from_numpy(G["uv"]))
    del errs["u"]
    print({k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v <= 1e-10 for v in errs.values()), errs


def test_fp64_host_compile_agrees_with_golden_and_oracle(G, gold, mp_blocks):
    K, X, p, uv = [t.numpy() for t in golden_inputs(G)]
    r, J = hostmath_bal_core(K, X, p, uv)
    u, _ = hostmath_bal_core(K, X, p, None)
    r_mp, JK, JX, Jp = [torch.from_numpy(a) for a in mp_blocks]
    for name, ref in (("golden", gold), ("oracle", (r_mp + torch.from_numpy(uv), r_mp, JK, JX, Jp))):
        errs = errors(u, r, J, ref, torch.from_numpy(uv))
        print(name, {k: f"{v:.2e}" for k, v in errs.items()})
        assert all(v <= GATE[F64] for v in errs.values()), (name, errs)
    assert np.array_equal(hostmath_bal_core(K, X, p, uv)[0], r) and np.array_equal(hostmath_bal_core(K, X, p, None)[1], J)


@pytest.mark.parametrize("source", ["golden", "wide"])
def test_fp32_host_compile_within_the_fp32_rule(G, source):
    host = golden_inputs(G, torch.float32) if source == "golden" else list(wide_inputs(2 * TILE + 3, torch.float32))
    ref_errs, ref = formula_errors(host)
    K, X, p, uv = [t.numpy() for t in host]
    r, J = hostmath_bal_core(K, X, p, uv)
    u, _ = hostmath_bal_core(K, X, p, None)
    out, ok = fp32_rule(errors(u, r, J, ref, host[3]), ref_errs)
    print(source, {k: f"{e:.2e} (bound {b:.2e}, x{q:.2f} of the formula)" for k, (e, b, q) in out.items()})
    assert ok, out


def test_fp64_host_compile_on_wide_inputs():
    host = wide_inputs(2 * TILE + 3, F64)
    K, X, p, uv = [t.numpy() for t in host]
    r, J = hostmath_bal_core(K, X, p, uv)
    u, _ = hostmath_bal_core(K, X, p, None)
    errs = errors(u, r, J, reference(*host), host[3])
    assert all(v <= GATE[F64] for v in errs.values()), errs


def test_composed_route_on_host_tensors_reproduces_the_golden(G, gold):
    K, X, p, uv = golden_inputs(G)
    with oracle_backend():
        leaves = [K.clone().requires_grad_(True), pp.Parameter(pp.SE3(X.clone())), p.clone().requires_grad_(True)]
        r = pp.bal_reprojerr(leaves[2], uv, leaves[0], leaves[1])
        rows = [torch.autograd.grad(r[:, a].sum(), leaves, retain_graph=True) for a in range(2)]
        u = pp.bal_point2pixel(p, K, pp.SE3(X))
    gX = torch.stack([torch.Tensor.as_subclass(rows[a][1], torch.Tensor) for a in range(2)], 1)
    assert float(gX[..., 6].abs().max()) == 0
    J = torch.cat([torch.stack([rows[0][0], rows[1][0]], 1), gX[..., :6], torch.stack([rows[0][2], rows[1][2]], 1)], -1)
    errs = errors(u, r.detach(), J, gold, uv)
    print({k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v <= 1e-9 for v in errs.values()), errs


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_vjp_is_g_times_J(G, dtype):
    K, X, p, uv = [G[k].astype(dtype) for k in ("K", "X", "p", "uv")]
    _, J = hostmath_bal_core(K, X, p, uv)
    g = np.random.default_rng(1).standard_normal((len(K), 2)).astype(dtype)
    gK, gX, gp = hostmath_bal_vjp(J, g)
    Jm = J.reshape(-1, 2, 12)
    want = g[:, 0:1] * Jm[:, 0] + g[:, 1:2] * Jm[:, 1]            # the same two products and one sum: equal to the last bit
    assert np.array_equal(gK, want[:, 0:3]) and np.array_equal(gX[:, :6], want[:, 3:9]) and np.array_equal(gp, want[:, 9:12])
    assert np.array_equal(gX[:, 6], np.zeros(len(K), dtype)) and not np.signbit(gX[:, 6]).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_zero_depth_is_non_finite_but_not_the_composed_pattern(dtype):
    """A zero depth: the closed form and the composed model both return a non-finite residual, not the same one.  With
    rho = inf the Horner form 1 + rho (k1 + k2 rho) of bal_math.h is -+inf where 1 + k1 rho + k2 rho^2 is inf - inf = nan."""
    eye = np.array([[0, 0, 0, 0, 0, 0, 1]] * 4, dtype)
    p = np.array([[0.3, -0.2, 0]] * 2 + [[0, 0, 0]] * 2, dtype)
    K = np.array([[500, 0.1, -0.01], [500, -0.1, 0.01]] * 2, dtype)
    r, J = hostmath_bal_core(K, eye, p, np.zeros((4, 2), dtype))
    assert not np.isfinite(r).any()
    assert np.isinf(r[:2]).all() and np.isnan(r[2:]).all()                       # d = -inf / +inf: +-inf, no nan; 0 / 0: nan
    with oracle_backend():
        rc = pp.bal_reprojerr(torch.from_numpy(p), torch.zeros(4, 2, dtype=torch.from_numpy(p).dtype), torch.from_numpy(K),
                              pp.SE3(torch.from_numpy(eye)))
    assert not torch.isfinite(rc).any() and torch.isnan(rc).all()
    assert not np.isfinite(J.reshape(4, 2, 12)[:, :, 3:]).all(axis=(1, 2)).any()

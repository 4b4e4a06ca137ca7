"""Point-eliminated PCG (SchurPCG) through csrc/ba_schur.hip on the MI355X: operators against the dense fp64 reference, run-to-run
bits, the solve through MultiGraphLinearization.solve, the fall-backs, and the reference's LM trajectory."""
import numpy as np
import pytest
import torch

import pypose_amd as pp
from pypose_amd.optim import multigraph
from tests import ba_schur_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_cache = {}


def case(mb):
    """(problem, x, dense fp64 reference, error of the tensor formulation evaluated in fp32 on the host), computed once"""
    if mb not in _cache:
        P = U.problem(mb)
        xc = torch.randn(U.NC * mb, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
        want = U.reference_operators(P, xc)
        lin32, shift32 = U.linearization(P, torch.float32, "cpu")
        t32 = U.operators(lin32.schur_pcg_ops(shift32), P, xc)
        _cache[mb] = (P, xc, want, {k: ((t32[k] - want[k]).abs().max() / want[k].abs().max()).item() for k in want})
    return _cache[mb]


@pytest.mark.parametrize("name", ["Sx", "bS", "Scc", "Minv_x", "back"])
@pytest.mark.parametrize("mb", [6, 9])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_operators_match_dense_reference(dtype, mb, name):
    """fp64: 1e-12 of the reference's max-abs.  fp32: max(2e-5, 4 x E_ref), E_ref the error of the tensor formulation in fp32 on
    the same inputs (Pi cancels at small damping: no fixed gate is derivable)."""
    P, xc, want, eref = case(mb)
    lin, shift = U.linearization(P, dtype, DEV)
    ops = lin.schur_pcg_ops(shift)
    assert isinstance(ops, multigraph._SchurHip)
    got = U.operators(ops, P, xc)[name]
    err = ((got - want[name]).abs().max() / want[name].abs().max()).item()
    gate = 1e-12 if dtype == torch.float64 else max(2e-5, 4 * eref[name])
    print(f"ba_schur {name} mb={mb} {dtype}: err {err:.3e} E_ref {eref[name]:.3e} ratio {err / eref[name]:.2f} gate {gate:.3e}")
    assert err <= gate


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_S_is_bit_reproducible(dtype):
    P, xc, _, _ = case(9)
    lin, shift = U.linearization(P, dtype, DEV)
    ops = lin.schur_pcg_ops(shift)
    x = xc.to(dtype).to(DEV).view(U.NC, 9)
    assert torch.equal(ops.S(x), ops.S(x))


def full_residual(P, D, mb):
    """relative residual of the flat step in the dense damped full system (LM's clamp and damping 1e-2 on the diagonal)"""
    diag = (P["J"] ** 2).sum(0)
    ref = U.reference(P, shift=1.01 * diag.clamp(1e-6, 1e32) - diag)
    D, n, cols, off = D.double().cpu().reshape(-1), U.NC * mb, [], 0
    for w in U.KEPT[mb]:
        cols.append(D[off:off + U.NC * w].view(U.NC, w))
        off += U.NC * w
    d = torch.cat([torch.cat(cols, -1).reshape(-1), D[n:]])
    return (torch.linalg.norm(ref["H"] @ d + ref["g"]) / torch.linalg.norm(ref["g"])).item()


def solve(mb, precond, weighted=False):
    P = case(mb)[0] if mb in (6, 9) else U.problem(mb)
    W = torch.eye(2, dtype=torch.float64).repeat(P["E"], 1, 1) if weighted else None
    lin, _ = U.linearization(P, torch.float64, DEV, W)
    lin.build_normal_equations(1e-6, 1e32)
    lin.damp(1e-2)
    solver = pp.optim.solver.SchurPCG(tol=1e-12, precond=precond)
    res = full_residual(P, lin.solve(solver), mb)
    print(f"ba_schur solve mb={mb} {precond} weighted={weighted}: {solver.iterations} iterations, full residual {res:.3e}")
    return lin, res


@pytest.mark.parametrize("precond", ["schur", "jacobi"])
@pytest.mark.parametrize("mb", [6, 9])
def test_solve_through_the_linearization(mb, precond):
    lin, res = solve(mb, precond)
    assert res <= 1e-9
    assert lin.opt._last_solve == "schur-pcg" and isinstance(lin._schur_ops[1], multigraph._SchurHip)


def test_fallbacks_report_their_route():
    lin, res = solve(9, "schur", weighted=True)               # a weight: the full-system PCG
    assert res <= 1e-9 and lin.opt._last_solve == "pcg"
    lin, res = solve(5, "schur")                              # a kept width the kernels do not take: the tensor formulation
    assert res <= 1e-9 and lin.opt._last_solve == "schur-pcg" and isinstance(lin._schur_ops[1], multigraph._SchurTensor)


def test_lm_trajectory_matches_reference():
    from tests.optim_models import ba_case, load_ba_golden, run_steps
    G = load_ba_golden()
    model, opt, args = ba_case(G, "ba_small", DEV)
    opt.solver = pp.optim.solver.SchurPCG(tol=1e-14, maxiter=5000)
    rec = run_steps(opt, (args,), {}, 3)
    assert set(rec["kind"]) == {"multigraph"} and opt._last_solve == "schur-pcg"
    assert any(k[0] == "schur-pcg" for k in opt._pcg_workspaces)
    np.testing.assert_allclose(rec["loss"][:3], G["ba_small/loss"][:3], rtol=1e-6)

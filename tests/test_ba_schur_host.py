"""Point-eliminated PCG (SchurPCG), device-agnostic formulation: the operators and the solve against the dense fp64 algebra,
and the group detection shared with the dense Schur route."""
import pytest
import torch

import pypose_amd as pp
from pypose_amd.optim import multigraph
from tests import ba_schur_util as U


@pytest.mark.parametrize("mb", [6, 9])
@pytest.mark.parametrize("name", ["Sx", "bS", "Scc", "Minv_x", "back"])
def test_tensor_operators_match_dense_reference(mb, name):
    P = U.problem(mb)
    xc = torch.randn(U.NC * mb, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    lin, shift = U.linearization(P, torch.float64, "cpu")
    got, want = U.operators(lin.schur_pcg_ops(shift), P, xc)[name], U.reference_operators(P, xc)[name]
    assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()


@pytest.mark.parametrize("precond", ["schur", "jacobi"])
@pytest.mark.parametrize("mb", [6, 9])
def test_solve_through_the_linearization(mb, precond):
    P = U.problem(mb)
    lin, _ = U.linearization(P, torch.float64, "cpu")
    lin.build_normal_equations(1e-6, 1e32)
    lin.damp(1e-2)
    solver = pp.optim.solver.SchurPCG(tol=1e-12, precond=precond)
    D = lin.solve(solver).reshape(-1)
    assert lin.opt._last_solve == "schur-pcg" and solver.iterations > 0
    diag = (P["J"] ** 2).sum(0)
    ref = U.reference(P, shift=1.01 * diag.clamp(1e-6, 1e32) - diag)          # what LM's clamp and damping add to the diagonal
    # flat step: parameter by parameter; the reference: camera rows [kept slots], then points
    n, cols, off = U.NC * mb, [], 0
    for w in U.KEPT[mb]:
        cols.append(D[off:off + U.NC * w].view(U.NC, w))
        off += U.NC * w
    d = torch.cat([torch.cat(cols, -1).reshape(-1), D[n:]])
    assert torch.linalg.norm(ref["H"] @ d + ref["g"]).item() <= 1e-9 * torch.linalg.norm(ref["g"]).item()


def test_group_detection_gives_schur_plan_the_same_plan():
    """ba_small's index structure (K and C by camera, P by point): the plan of the dense Schur route is what it was"""
    from tests.optim_models import load_ba_golden
    G = load_ba_golden()
    cidx, pidx = torch.as_tensor(G["ba_small/cidx"]).long(), torch.as_tensor(G["ba_small/pidx"]).long()
    E, Nc, Np = cidx.numel(), G["ba_small/K0"].shape[0], G["ba_small/P0"].shape[0]
    params = [torch.zeros(Nc, 3, dtype=torch.float64), torch.zeros(Nc, 6, dtype=torch.float64), torch.zeros(Np, 3, dtype=torch.float64)]
    slots = [(k, idx, torch.randn(E, 2, params[k].shape[-1], dtype=torch.float64)) for k, idx in enumerate((cidx, cidx.clone(), pidx))]
    lin = multigraph.MultiGraphLinearization(U.Opt(), None, torch.randn(E, 2, dtype=torch.float64), params, slots)
    plan = lin.schur_plan()
    assert (plan["a"], plan["b"], plan["Na"], plan["Nb"]) == ([2], [0, 1], Np, Nc)
    grp = lin.bipartite_groups()
    assert (grp["a"], grp["b"], grp["ma"], grp["mb"]) == ([2], [0, 1], 3, 9)
    lin.slots.append((2, cidx, slots[2][2]))              # a parameter in two slots: not bipartite
    del lin._groups
    assert lin.bipartite_groups() is None


def test_lm_takes_the_route_on_the_reference_problem():
    """the reference's recorded dense trajectory on ba_small, through the stand-in back end"""
    import numpy as np
    from tests.optim_models import ba_case, load_ba_golden, run_steps
    from tests.oracle_backend import oracle_backend
    G = load_ba_golden()
    with oracle_backend():
        model, opt, args = ba_case(G, "ba_small")
        opt.solver = pp.optim.solver.SchurPCG(tol=1e-14, maxiter=5000)
        rec = run_steps(opt, (args,), {}, 3)
    assert opt._last_solve == "schur-pcg"
    np.testing.assert_allclose(rec["loss"][:3], G["ba_small/loss"][:3], rtol=1e-6)

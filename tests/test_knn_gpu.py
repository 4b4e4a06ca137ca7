"""csrc/knn.hip on the MI355X: pp.knn against a brute-force fp64 distance matrix on the same (already rounded) inputs, ties,
the ICP statistics and pp.module.ICP end to end, and the gradient route."""
import functools

import pytest
import torch

import pypose_amd as pp
from pypose_amd.function import geometry as geo
from tests.test_knn_host import icp_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (batch of ref, N1, N2, forced S): either side of the 256-lane block and of the 1024-point tile, a ragged last split, and a
# batch of three against ONE shared neighbour cloud (stride 0)
CASES = [(1, 1, 16, None), (1, 255, 1023, None), (1, 257, 1025, None), (1, 300, 5000, 3), (3, 257, 1025, None)]


@functools.lru_cache(maxsize=None)
def reference(case, dtype, grid=False):
    """(ref, nbr) in ``dtype`` and the fp64 distance matrix of the rounded clouds, stably sorted: (values, indices)"""
    B, n1, n2, _ = case
    g = torch.Generator().manual_seed(n1 + n2)
    if grid:        # a small integer grid with many duplicated points: distances are exact in fp32, ties everywhere
        ref, nbr = torch.randint(0, 3, (B, n1, 3), generator=g).to(dtype), torch.randint(0, 3, (n2, 3), generator=g).to(dtype)
    else:
        ref, nbr = torch.randn(B, n1, 3, generator=g).to(dtype), torch.randn(n2, 3, generator=g).to(dtype)
    dist = torch.linalg.norm(ref.double().unsqueeze(-2) - nbr.double(), dim=-1)
    return (ref, nbr) + tuple(torch.sort(dist, dim=-1, stable=True))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_values_and_indices(dtype, k, case):
    """|values - ref| <= 4 eps ref (three roundings in d^2 and the square root stay under 2 eps; identical points give exactly
    0), and the fp64 distance to nbr[index] meets the same bound (topk leaves ties open: indices are compared in test_ties)."""
    ref, nbr, want, _ = reference(case, dtype)
    out = pp.knn(ref.to(DEV), nbr.to(DEV), k=k, _splits=case[3])
    values, indices = out.values.cpu().double(), out.indices.cpu()
    assert out.values.dtype == dtype and indices.dtype == torch.int64 and values.shape == ref.shape[:-1] + (k,)
    bound = 4 * torch.finfo(dtype).eps * want[..., :k]
    assert ((values - want[..., :k]).abs() <= bound).all()
    assert (indices >= 0).all() and (indices < nbr.shape[0]).all()
    picked = torch.linalg.norm(ref.double().unsqueeze(-2) - nbr.double()[indices], dim=-1)
    assert ((picked - want[..., :k]).abs() <= bound).all()


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("k", [3, 16])
def test_ties_keep_the_smaller_index(k, splits):
    ref, nbr, _, order = reference(CASES[3], torch.float32, True)
    out = pp.knn(ref.to(DEV), nbr.to(DEV), k=k, _splits=splits)
    assert torch.equal(out.indices.cpu(), order[..., :k])


def icp_reference(dtype):
    """the fixture in ``dtype`` on the device, the true transform as an SE3 row, and the fp64 sums over the fp64 association"""
    source, target, R, t, perm = icp_fixture()
    src, tgt = source.to(dtype).to(DEV), target.to(dtype).to(DEV)
    T = pp.mat2SE3(torch.cat((R, t.unsqueeze(-1)), -1).to(DEV), check=False).tensor().to(dtype).view(1, 7)
    p = pp.SE3(T.double()).Act(src.double())
    dist, order = torch.sort(torch.linalg.norm(p.unsqueeze(-2) - tgt.double(), dim=-1), dim=-1)
    assert torch.equal(order[:, 0].cpu(), perm) and ((dist[:, 1] - dist[:, 0]) / dist[:, 1]).min() >= 0.5      # no near-tie
    q = tgt.double()[order[:, 0]]
    terms = torch.cat([dist[:, :1], p, q, (q.unsqueeze(-1) * p.unsqueeze(-2)).reshape(-1, 9)], -1)
    return src, tgt, T, order[:, 0], terms.sum(0), terms.abs().sum(0)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_icp_statistics(dtype):
    """fp64: 1e-12 of the sum of absolute terms.  fp32: max(1e-5, 4 x E_ref), 1e-5 the fp32 row gate of this project and E_ref
    the error of the fp32 tensor formulation (SE3.Act, gather, sums) on the same rows.  Two runs give the same bits."""
    src, tgt, T, match, want, scale = icp_reference(dtype)
    got = geo._icp_stats(src, 0, tgt, 0, T, 1, {})
    assert got.dtype == torch.float64 and torch.equal(got, geo._icp_stats(src, 0, tgt, 0, T, 1, {}))
    err = ((got[0] - want).abs() / scale).max().item()
    gate = 1e-12
    if dtype == torch.float32:
        p, q = pp.SE3(T).Act(src), tgt[match]
        terms = torch.cat([torch.linalg.norm(p - q, dim=-1, keepdim=True), p, q, (q.unsqueeze(-1) * p.unsqueeze(-2)).reshape(-1, 9)], -1)
        eref = ((terms.sum(0).double() - want).abs() / scale).max().item()
        gate = max(1e-5, 4 * eref)
        print(f"icp stats fp32: err {err:.3e} E_ref {eref:.3e} ratio {err / eref:.2f} gate {gate:.3e}")
    assert err <= gate


@functools.lru_cache(maxsize=None)
def icp_result(dtype, route):
    """the SE3 row of ICP on the fixture: the kernel route or, with the route test switched off, the loop over the tensors"""
    source, target = icp_fixture()[:2]
    icp = pp.module.ICP(stepper=pp.utils.ReduceToBason(steps=6, patience=6))
    taken = geo._knn_on_kernels
    try:
        if route == "tensors":
            geo._knn_on_kernels = lambda *a: False
        return icp(source.to(dtype).to(DEV), target.to(dtype).to(DEV))
    finally:
        geo._knn_on_kernels = taken


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_icp_end_to_end(dtype):
    """within 1e-3 (the noise) of the true transform; fp64: the tensor route's result within 1e-9; fp32: against the fp64 result,
    max(1e-5, 4 x E_ref) with E_ref the fp32 tensor route's error."""
    _, _, R, t, _ = icp_fixture()
    got = icp_result(dtype, "kernels")
    M = got.matrix().cpu().double()
    assert (M[:3, :3] - R).abs().max() <= 1e-3 and (M[:3, 3] - t).abs().max() <= 1e-3
    want = icp_result(torch.float64, "tensors").tensor()
    err = (got.tensor().double() - want).abs().max().item()
    gate = 1e-9
    if dtype == torch.float32:
        eref = (icp_result(dtype, "tensors").tensor().double() - want).abs().max().item()
        gate = max(1e-5, 4 * eref)
        print(f"icp fp32: err {err:.3e} E_ref {eref:.3e} ratio {err / eref:.2f} gate {gate:.3e}")
    assert err <= gate


def test_gradient_matches_the_tensor_formulation():
    ref, nbr = reference(CASES[2], torch.float64)[:2]
    grads = []
    for fn in (pp.knn, geo._knn_tensor):
        r, n = ref[0].to(DEV).requires_grad_(), nbr.to(DEV).requires_grad_()
        fn(r, n, 3, 2, -1, False, True).values.sum().backward()
        grads.append((r.grad, n.grad))
    assert (grads[0][0] - grads[1][0]).abs().max() <= 1e-12 and (grads[0][1] - grads[1][1]).abs().max() <= 1e-12

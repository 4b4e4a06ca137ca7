"""csrc/knn_grid.hip on the MI355X: pp.knn through a pp.knn_index against the fp64 distance matrix of the (already rounded)
clouds, stably sorted, and bit for bit against the brute-force route, on clouds that stress the cell box and its certification;
the ICP statistics and pp.module.ICP through the index; the public interface."""
import functools

import pytest
import torch

import pypose_amd as pp
from pypose_amd.function import geometry as geo
from tests.test_knn_gpu import CASES as BRUTE_CASES, icp_reference, icp_result, reference as brute_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CLOUDS = ["normal", "wide", "clustered", "outside", "planar", "small", "batched", "unordered", "lattice"]


@functools.lru_cache(maxsize=None)
def reference(cloud, dtype):
    """(ref, nbr) in ``dtype`` and the fp64 distance matrix of the rounded clouds, stably sorted: (values, indices)"""
    if cloud == "lattice":              # test_knn_gpu's integer lattice (300 x 5000): exact distances, ties everywhere
        return brute_reference(BRUTE_CASES[3], dtype, True)
    g = torch.Generator().manual_seed(CLOUDS.index(cloud))
    n1, n2 = (300, 5000) if cloud == "wide" else (257, 16) if cloud == "small" else (257, 1025)
    ref, nbr = torch.randn(3 if cloud == "batched" else 1, n1, 3, generator=g), torch.randn(n2, 3, generator=g)
    if cloud == "clustered":            # 90 % of the target in a ball of radius 0.01, the rest over [-10, 10]^3: most cells are empty
        ball = torch.nn.functional.normalize(nbr[:922]) * 0.01 * torch.rand(922, 1, generator=g) ** (1 / 3)
        nbr = torch.cat([ball, 20 * torch.rand(n2 - 922, 3, generator=g) - 10])
        ref = torch.cat([0.01 * ref[:, :128], 5 * ref[:, 128:]], 1)
    elif cloud == "outside":            # every query beyond the target's bounding box
        ref = ref + torch.tensor([30.0, 0.0, 0.0])
    elif cloud == "planar":             # a degenerate axis
        nbr[:, 2] = 0
    ref, nbr = ref.to(dtype), nbr.to(dtype)
    dist = torch.linalg.norm(ref.double().unsqueeze(-2) - nbr.double(), dim=-1)
    return (ref, nbr) + tuple(torch.sort(dist, dim=-1, stable=True))


@pytest.mark.parametrize("cloud", CLOUDS)
@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_index_against_fp64_and_brute_force(dtype, k, cloud):
    """test_knn_gpu's bound: |values - ref| <= 4 eps ref, and the fp64 distance to nbr[index] meets it too; on the lattice the
    indices equal the stable-sort order (the tie rule under out-of-order visits); everywhere the brute-force route's bits."""
    ref, nbr, want, order = reference(cloud, dtype)
    r, n = ref.to(DEV), nbr.to(DEV)
    out = pp.knn(r, pp.knn_index(n), k=k, _order=cloud != "unordered")
    values, indices = out.values.cpu().double(), out.indices.cpu()
    assert out.values.dtype == dtype and indices.dtype == torch.int64 and values.shape == ref.shape[:-1] + (k,)
    bound = 4 * torch.finfo(dtype).eps * want[..., :k]
    assert ((values - want[..., :k]).abs() <= bound).all()
    assert (indices >= 0).all() and (indices < nbr.shape[0]).all()
    picked = torch.linalg.norm(ref.double().unsqueeze(-2) - nbr.double()[indices], dim=-1)
    assert ((picked - want[..., :k]).abs() <= bound).all()
    if cloud == "lattice":
        assert torch.equal(indices, order[..., :k])
    brute = pp.knn(r, n, k=k)
    assert torch.equal(out.values, brute.values) and torch.equal(out.indices, brute.indices)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_icp_statistics_through_the_index(dtype):
    """the matches of the fp64 association, and test_icp_statistics' gates on the 16 sums"""
    src, tgt, T, match, want, scale = icp_reference(dtype)
    ws = {}
    got = geo._icp_stats(src, 0, tgt, 0, T, 1, ws, grid=(pp.knn_index(tgt), None))
    assert torch.equal(ws["pidx"].view(-1).long(), match)
    err = ((got[0] - want).abs() / scale).max().item()
    gate = 1e-12
    if dtype == torch.float32:
        p, q = pp.SE3(T).Act(src), tgt[match]
        terms = torch.cat([torch.linalg.norm(p - q, dim=-1, keepdim=True), p, q, (q.unsqueeze(-1) * p.unsqueeze(-2)).reshape(-1, 9)], -1)
        gate = max(1e-5, 4 * ((terms.sum(0).double() - want).abs() / scale).max().item())
    print(f"icp stats through the index {dtype}: err {err:.3e} gate {gate:.3e}")
    assert err <= gate


def test_icp_end_to_end_through_the_index(monkeypatch):
    """with the crossover forced to 0, the brute-force route's SE3 row to 1e-9 in fp64"""
    want = icp_result(torch.float64, "kernels").tensor()
    monkeypatch.setattr(geo, "_GRID_ICP_MIN_N2", 0)
    got = icp_result.__wrapped__(torch.float64, "kernels").tensor()
    assert (got - want).abs().max() <= 1e-9


def test_knn_index_refuses_a_host_cloud():
    with pytest.raises(ValueError):
        pp.knn_index(torch.randn(64, 3))


def test_gradient_matches_the_tensor_formulation():
    ref, nbr = reference("normal", torch.float64)[:2]
    grads = []
    for indexed in (True, False):
        r, n = ref[0].to(DEV).requires_grad_(), nbr.to(DEV).requires_grad_()
        out = pp.knn(r, pp.knn_index(n), k=3) if indexed else geo._knn_tensor(r, n, 3, 2, -1, False, True)
        out.values.sum().backward()
        grads.append((r.grad, n.grad))
    assert (grads[0][0] - grads[1][0]).abs().max() <= 1e-12 and (grads[0][1] - grads[1][1]).abs().max() <= 1e-12

"""csrc/nbr_grid.hip on the MI355X: pp.nbr_filter and pp.knn_filter through the grid index (``_grid=``) against the fp64 distance
matrix of the (already rounded) cloud and against the brute-force route, on clouds that stress the cell box and the stream."""
import functools

import pytest
import torch

import pypose_amd as pp
from pypose_amd.function import geometry as geo
from tests.test_cloud_filter_gpu import neighbours

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.float64]
# name -> (N, nbr); `whole` and `zero` (the lattice, radius 0) fix their radius, the others take the widest gap around r0
SHAPES = {"clustered": (3000, 2), "clustered-no-stop": (3000, 2600), "planar": (1025, 2), "fine": (5000, 2), "whole-all": (1025, 1024),
          "whole-none": (1025, 1025), "zero": (1025, 16)}


def both_routes(pts, nbr, radius, want, grid=True):
    """the grid route's mask and rows equal the fp64 ones and the brute-force route's"""
    x = pts.to(DEV)
    out, mask = pp.nbr_filter(x, nbr, radius, pdim=3, return_mask=True, _grid=grid)
    brute, bmask = pp.nbr_filter(x, nbr, radius, pdim=3, return_mask=True, _grid=False)
    assert mask.dtype == torch.bool and torch.equal(mask.cpu(), want) and torch.equal(out.cpu(), pts[want])
    assert torch.equal(mask, bmask) and torch.equal(out, brute)


@pytest.mark.parametrize("n, lattice", [(1, False), (255, False), (257, False), (1025, False), (5000, False), (1025, True)])
@pytest.mark.parametrize("D", [3, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_nbr_filter_mask_through_the_grid(dtype, D, n, lattice):
    pts, radius, count, _ = neighbours(n, D, dtype, lattice)
    nbr = 250 if lattice else 2        # (250: the pairs at exactly d = r decide for many points)
    want = count[0] - 1 >= nbr
    assert n < 255 or (want.any() and not want.all())
    both_routes(pts[0], nbr, radius, want)


@functools.lru_cache(maxsize=None)
def shaped(name, dtype):
    """cloud [N, 3] in ``dtype``, a radius with no pair within 1e-5 r of it, and the fp64 counts within it"""
    kind, n = name.split("-")[0], SHAPES[name][0]
    g = torch.Generator().manual_seed(n)
    pts, radius, r0 = torch.randn(n, 3, generator=g, dtype=torch.float64), None, 2.5 * n ** (-1 / 3)
    if kind == "clustered":            # 2700 points in a ball of radius 0.01 (one cell, a run of more than two LDS tiles), 300 far apart
        ball = torch.nn.functional.normalize(pts[:2700]) * 0.01 * torch.rand(2700, 1, generator=g, dtype=torch.float64) ** (1 / 3)
        pts, r0 = torch.cat([ball, 20 * torch.rand(n - 2700, 3, generator=g, dtype=torch.float64) - 10]), 0.05
    elif kind == "planar":             # a degenerate axis
        pts[:, 2] = 0
    elif kind == "fine":               # a slab 1e-3 thick: 1 x 128 x 128 cells at occupancy 1, most of them empty
        pts, r0 = torch.rand(n, 3, generator=g, dtype=torch.float64) * torch.tensor([1e-3, 1.0, 1.0]), 0.02
    elif kind == "whole":
        radius = 100.0
    elif kind == "zero":
        pts, radius = neighbours(n, 3, dtype, True)[0][0].double(), 0.0
    pts = pts.to(dtype)
    dist = torch.cdist(pts.double(), pts.double())
    if radius is None:                 # the fixture's rule: the middle of the widest gap between pair distances within 10 % of r0
        near = dist[(dist > 0.9 * r0) & (dist < 1.1 * r0)].sort().values
        near = torch.cat([near.new_tensor([0.9 * r0]), near, near.new_tensor([1.1 * r0])])
        j = (near[1:] - near[:-1]).argmax()
        radius = ((near[j] + near[j + 1]) / 2).item()
    assert kind == "zero" or not ((dist - radius).abs() <= 1e-5 * radius).any()
    return pts, radius, (dist <= radius).sum(-1)


@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_shapes_that_stress_the_box_and_the_stream(dtype, name):
    pts, radius, count = shaped(name, dtype)
    nbr = SHAPES[name][1]
    want = count - 1 >= nbr
    assert want.all() if name == "whole-all" else not want.any() if name == "whole-none" else want.any() and not want.all()
    grid = True
    if name == "fine":                 # every workgroup's box is 128 cells wide in y and >= 3 in z: more than kGridRuns runs
        grid = pp.knn_index(pts.to(DEV), _occupancy=1.0)
        h, gy = grid.header_host[0, 3].item(), grid.header_host[0, 5].item()
        ycell = ((grid.planes[1, :256] - pts[:, 1].min().item()) / h).floor()        # of the first workgroup's own points
        assert radius > h and gy == 128 and 3 * (ycell.max() - ycell.min() + 1) > 256
    both_routes(pts, nbr, radius, want, grid)


@pytest.mark.parametrize("lattice", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_counts_with_the_stop_disabled(dtype, lattice):
    pts, radius, count, _ = neighbours(1025 if lattice else 5000, 3, dtype, lattice)
    index = pp.knn_index(pts[0].to(DEV))
    got = geo._nbr_counts_grid(index, geo._radius2(radius, dtype), 2 ** 31 - 1, 1, pts.shape[1])
    assert got.dtype == torch.int32 and torch.equal(got.view(-1).cpu().long(), count[0])


KNN_CASES = [(n, D, k, r, 1) for n in (257, 1025, 5000) for D in (3, 6) for k in (1, 3, 15) for r in (False, True)] + [(257, 6, 3, False, 3)]


@pytest.mark.parametrize("n, D, k, with_radius, batch", KNN_CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_knn_filter_through_the_grid(dtype, n, D, k, with_radius, batch):
    """test_cloud_filter_gpu's bound, |out - want| <= (k + 3) eps max|x|, and the brute-force route's bits: the lists are
    bit-identical and the finish kernel is the same"""
    pts, radius, count, order = neighbours(n, D, dtype, batch=batch, wide=k == 15)
    x = pts.to(DEV) if batch > 1 else pts[0].to(DEV)
    kwargs = dict(k=k, pdim=3, radius=radius if with_radius else None)
    want = pts.double()[torch.arange(batch).view(-1, 1, 1), order[..., :k + 1]].mean(dim=-2)
    keep = count[0] - 1 >= k
    assert not with_radius or (keep.any() and not keep.all())
    want = want[0][keep] if with_radius else want if batch > 1 else want[0]
    out = pp.knn_filter(x, _grid=True, **kwargs)
    assert out.dtype == dtype and out.shape == want.shape
    assert ((out.cpu().double() - want).abs() <= (k + 3) * torch.finfo(dtype).eps * pts.abs().max().item()).all()
    assert torch.equal(out, pp.knn_filter(x, _grid=False, **kwargs))

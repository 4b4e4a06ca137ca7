"""csrc/cloud_filter.hip on the MI355X: pp.nbr_filter, pp.knn_filter and pp.voxel_filter against plain fp64 references computed on
the CPU from the same (already rounded) inputs."""
import functools

import pytest
import torch

import pypose_amd as pp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.float64]
# (N, forced S): either side of the 256-lane block and of the 1024-point tile, a ragged last split, and three tiles in ONE split
# (both LDS buffers reused)
SIZES = [(1, None), (255, None), (257, None), (1025, None), (5000, 3), (2049, 1)]


@functools.lru_cache(maxsize=None)
def neighbours(n, D, dtype, lattice=False, batch=1, wide=False):
    """cloud [batch, n, D] in ``dtype``, a radius, and from the fp64 distance matrix of its first three columns: the count within
    the radius (the point itself included) and the 16 nearest indices, stably sorted (``wide``: twice the radius, about thirty
    neighbours inside).  No pair lies within 1e-5 r of the radius (on the lattice -- integer coordinates in [0, 4)^3, radius 2 -- pairs at exactly d^2 = r^2 exist and are exact in fp32)."""
    g = torch.Generator().manual_seed(n + D)
    if lattice:
        pts = torch.randint(0, 4, (batch, n, D), generator=g).to(dtype)
    else:
        pts = torch.randn(batch, n, D, generator=g, dtype=torch.float64).to(dtype)
    xyz = pts[..., :3].double()
    dist = torch.linalg.norm(xyz.unsqueeze(-2) - xyz.unsqueeze(-3), dim=-1)
    radius = 2.0
    if not lattice:      # the middle of the widest gap between pair distances within 10 % of the median nearest-pair scale
        r0 = (5.0 if wide else 2.5) * n ** (-1 / 3)
        near = dist[(dist > 0.9 * r0) & (dist < 1.1 * r0)].sort().values
        near = torch.cat([near.new_tensor([0.9 * r0]), near, near.new_tensor([1.1 * r0])])
        j = (near[1:] - near[:-1]).argmax()
        radius = ((near[j] + near[j + 1]) / 2).item()
    assert lattice or not ((dist - radius).abs() <= 1e-5 * radius).any()
    return pts, radius, (dist <= radius).sum(-1), torch.sort(dist, dim=-1, stable=True).indices[..., :16]


@pytest.mark.parametrize("n, splits, lattice", [s + (False,) for s in SIZES] + [(1025, None, True)])
@pytest.mark.parametrize("D", [3, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_nbr_filter_mask_is_the_fp64_one(dtype, D, n, splits, lattice):
    pts, radius, count, _ = neighbours(n, D, dtype, lattice)
    nbr = 250 if lattice else 2        # (250: the pairs at exactly d = r decide for many points)
    want = count[0] - 1 >= nbr
    assert n < 255 or (want.any() and not want.all())
    out, mask = pp.nbr_filter(pts[0].to(DEV), nbr, radius, pdim=3, return_mask=True, _splits=splits)
    assert mask.dtype == torch.bool and torch.equal(mask.cpu(), want) and torch.equal(out.cpu(), pts[0][want])


@pytest.mark.parametrize("n, splits", SIZES)
@pytest.mark.parametrize("k", [1, 3, 15])
@pytest.mark.parametrize("with_radius", [False, True])
@pytest.mark.parametrize("D", [3, 6])
@pytest.mark.parametrize("dtype", DTYPES)
def test_knn_filter(dtype, D, with_radius, k, n, splits):
    check_knn_filter(dtype, D, with_radius, k, n, splits, 1)


def test_knn_filter_batched():
    check_knn_filter(torch.float32, 6, False, 3, 257, None, 3)


def check_knn_filter(dtype, D, with_radius, k, n, splits, batch):
    """|out - want| <= (k + 3) eps max|x|: k + 1 terms summed and one division (the fp64 accumulation stays well inside); with a
    radius some rows survive and some do not (k = 15 takes the wide radius for that)"""
    pts, radius, count, order = neighbours(n, D, dtype, batch=batch, wide=k == 15)
    x = pts.to(DEV) if batch > 1 else pts[0].to(DEV)
    kwargs = dict(k=k, pdim=3, radius=radius if with_radius else None, _splits=splits)
    if k + 1 > n:
        with pytest.raises(RuntimeError, match="out of range"):
            pp.knn_filter(x, **kwargs)
        return
    rows = torch.arange(batch).view(-1, 1, 1)
    want = pts.double()[rows, order[..., :k + 1]].mean(dim=-2)
    keep = count[0] - 1 >= k
    assert not with_radius or (keep.any() and not keep.all())
    want = want[0][keep] if with_radius else want if batch > 1 else want[0]
    out = pp.knn_filter(x, **kwargs)
    assert out.dtype == dtype and out.shape == want.shape
    assert ((out.cpu().double() - want).abs() <= (k + 3) * torch.finfo(dtype).eps * pts.abs().max().item()).all()


# name -> (N, coordinates, voxel): one cell; one run through five waves; one run across several workgroups (the carry path); almost
# all singletons; mixed run lengths crossing wave and workgroup boundaries; points exactly on cell edges with exact quotients; and
# (fp64) multiples of 0.1, where the float32 rounding of the voxel size decides the cell
CLOUDS = {"one": (1, "randn", [1., 1., 1.]), "waves": (257, "randn", [10., 10., 10.]), "carry": (3000, "randn", [1e3] * 3),
          "singletons": (1025, "randn100", [0.1] * 3), "mixed": (5000, "randn", [0.5, 0.25, 1.0]), "edges": (1025, "quarters", [0.5] * 3),
          "tenths": (1025, "tenths", [0.1] * 3)}
VOXEL_CASES = [(c, t) for c in CLOUDS if c != "tenths" for t in DTYPES] + [("tenths", torch.float64)]


@functools.lru_cache(maxsize=None)
def voxels(name, D, dtype):
    """cloud [N, D], its voxel sizes, and from CPU torch: every point's cell rank (cells computed in ``dtype`` with the same
    subtract / divide / truncate, grouped by torch.unique), the fp64 means and the populations"""
    n, kind, voxel = CLOUDS[name]
    g = torch.Generator().manual_seed(n + D)
    pts = torch.randn(n, D, generator=g, dtype=torch.float64)
    if kind == "randn100":
        pts = pts * 100
    elif kind != "randn":
        pts[:, :3] = torch.randint(0, 16 if kind == "quarters" else 50, (n, 3), generator=g) / (4. if kind == "quarters" else 10.)
    pts = pts.to(dtype)
    cells = ((pts[:, :3] - pts[:, :3].min(0).values) / torch.tensor(voxel, dtype=torch.float32)).to(torch.int64)
    uniq, inverse, counts = torch.unique(cells, dim=0, return_inverse=True, return_counts=True)
    means = torch.zeros(len(uniq), D, dtype=torch.float64).index_add_(0, inverse, pts.double()) / counts.view(-1, 1)
    return pts, voxel, inverse, means, counts


@pytest.mark.parametrize("name, dtype", VOXEL_CASES)
@pytest.mark.parametrize("D", [3, 5])
def test_voxel_filter(D, name, dtype):
    """same M, same row order, means within 2 eps max|x| (fp32: fp64 sums rounded once) or (c + 1) eps max|x| (fp64: c the
    cell's population); a second call gives the same bits"""
    pts, voxel, _, want, counts = voxels(name, D, dtype)
    out = pp.voxel_filter(pts.to(DEV), voxel)
    assert out.dtype == dtype and out.shape == want.shape
    terms = 2 if dtype == torch.float32 else counts.view(-1, 1) + 1
    assert ((out.cpu().double() - want).abs() <= terms * torch.finfo(dtype).eps * pts.abs().max().item()).all()
    assert torch.equal(out, pp.voxel_filter(pts.to(DEV), voxel))


@pytest.mark.parametrize("dtype", DTYPES)
def test_voxel_filter_random_picks_a_member_of_every_cell(dtype):
    pts, voxel, inverse, want, _ = voxels("mixed", 5, dtype)
    out = pp.voxel_filter(pts.to(DEV), voxel, random=True).cpu()
    assert out.shape == want.shape
    same = (out.unsqueeze(1) == pts.unsqueeze(0)).all(-1)                              # [M, N]
    assert (same & (inverse.unsqueeze(0) == torch.arange(len(out)).unsqueeze(1))).any(1).all()


@pytest.mark.parametrize("voxel", [[0.5, 0.25], [1e-7, 1., 1.]])
def test_clouds_outside_the_kernel_route_take_the_tensor_route_on_the_device(voxel):
    """vdim = 2, and a cell index past 21 bits (the flag read together with M): the tensor formulation, whose sums on the device
    are atomic -- (c + 1) eps max|x| against the CPU's"""
    pts = voxels("mixed", 5, torch.float64)[0][:257]
    want, out = pp.voxel_filter(pts, voxel), pp.voxel_filter(pts.to(DEV), voxel)
    assert out.is_cuda and out.shape == want.shape
    assert ((out.cpu() - want).abs() <= 258 * torch.finfo(torch.float64).eps * pts.abs().max().item()).all()

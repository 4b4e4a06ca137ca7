"""pp.nbr_filter / random_filter / voxel_filter / knn_filter on host tensors (the tensor route): the reference's doc-string examples
and the cases of its tests/function/test_downsample.py, with its expected values."""
import pytest
import torch

import pypose_amd as pp
from pypose_amd.function import geometry as geo

CLOUD = torch.tensor([[0., 0., 0.], [1., 0., 0.], [0., 1., 0.], [0., 1., 1.], [10., 1., 1.], [10., 1., 10.]])
CLOUD2 = torch.tensor([[1., 0., 0.], [1., 0., 0.], [0., 1., 0.], [4., 1., 1.], [10., 1., 1.], [1., 1., 10.]])
LINE = torch.tensor([[1., 2., 3.], [4., 5., 6.], [7., 8., 9.], [10., 11., 12.], [13., 14., 15.]])
CELLS = [[0., 0., 0.], [0., 1., 0.], [0., 1., 1.], [1., 0., 0.], [10., 1., 1.], [10., 1., 10.]]       # CLOUD in cell order


@pytest.mark.parametrize("kwargs, kept", [
    (dict(nbr=2, radius=5), [1, 1, 1, 1, 0, 0]), (dict(nbr=2, radius=12), [1, 1, 1, 1, 1, 0]),
    (dict(nbr=2, radius=10, pdim=2), [1, 1, 1, 1, 1, 1]), (dict(nbr=2, radius=10, pdim=3), [1, 1, 1, 1, 1, 0]),
    (dict(nbr=2, radius=2, ord=1), [1, 1, 1, 1, 0, 0]), (dict(nbr=0, radius=-1.), [0, 0, 0, 0, 0, 0])])
def test_nbr_filter(kwargs, kept, monkeypatch):
    monkeypatch.setattr(geo, "_KNN_CHUNK", 6 * 3 * 4)                  # four rows per chunk
    mask = torch.tensor(kept, dtype=torch.bool)
    out, got = pp.nbr_filter(CLOUD, return_mask=True, **kwargs)
    assert torch.equal(got, mask) and torch.equal(out, CLOUD[mask]) and torch.equal(pp.nbr_filter(CLOUD, **kwargs), CLOUD[mask])


@pytest.mark.parametrize("D", [3, 2])
def test_random_filter(D):
    points = torch.randn(5, 10, D)
    out = pp.random_filter(points, 5)
    assert out.shape == (5, 5, D)
    rows = (out[0].unsqueeze(1) == points[0]).all(-1)                  # [num, N]: every row once, the same draw in every batch
    assert (rows.sum(1) == 1).all() and (rows.sum(0) <= 1).all() and torch.equal(out[1], points[1][rows.float().argmax(1)])
    with pytest.raises(AssertionError):
        pp.random_filter(points, 11)


@pytest.mark.parametrize("points, voxel, want", [
    (LINE, [5., 5., 5.], [[2.5, 3.5, 4.5], [8.5, 9.5, 10.5], [13., 14., 15.]]),
    (LINE[:, :2], [5., 5.], [[2.5, 3.5], [8.5, 9.5], [13., 14.]]),
    (LINE[:, :2], [5.], [[2.5, 3.5], [8.5, 9.5], [13., 14.]]),
    (CLOUD, [1., 1., 1.], CELLS),
    (torch.cat([CLOUD, torch.zeros(6, 1)], -1), [1., 1., 1.], [c + [0.] for c in CELLS]),
    (torch.cat([LINE[:, :2], torch.zeros(5, 2)], -1), [5., 5., 1, 1], [[2.5, 3.5, 0, 0], [8.5, 9.5, 0, 0], [13., 14., 0, 0]]),
    (LINE.double(), [-5., 5., 5.], [[13., 14., 15.], [8.5, 9.5, 10.5], [2.5, 3.5, 4.5]])])
def test_voxel_filter(points, voxel, want):
    out = pp.voxel_filter(points, voxel)
    assert out.dtype == points.dtype and torch.equal(out, torch.tensor(want, dtype=points.dtype))


@pytest.mark.parametrize("points, voxel, cells", [(LINE, [5., 5., 5.], [[0, 1], [2, 3], [4]]), (LINE[:, :2], [5.], [[0, 1], [2, 3], [4]]),
                                                  (LINE[:, :2], [5., 1], [[0], [1], [2], [3], [4]])])
def test_voxel_filter_random_picks_a_member_of_every_cell(points, voxel, cells):
    for _ in range(4):
        out = pp.voxel_filter(points, voxel, random=True)
        assert out.shape == (len(cells), points.shape[1])
        assert all(any(torch.equal(row, points[i]) for i in cell) for row, cell in zip(out, cells))


def test_knn_filter():
    want = torch.tensor([[1 / 3, 1 / 3, 0.], [1 / 3, 1 / 3, 0.], [0., 2 / 3, 1 / 3], [0., 2 / 3, 1 / 3]])
    assert (pp.knn_filter(CLOUD, k=2, radius=5) - want).abs().max() <= 1e-6
    one, two = pp.knn_filter(CLOUD, k=2), pp.knn_filter(CLOUD2, k=2)
    assert (one[:4] - want).abs().max() <= 1e-6 and (one[4] - torch.tensor([7., 2 / 3, 11 / 3])).abs().max() <= 1e-6
    assert torch.equal(pp.knn_filter(torch.stack([CLOUD, CLOUD2]), k=2), torch.stack([one, two]))
    # survivors that are no prefix: the neighbours come from the whole cloud by original index
    flipped = CLOUD.flip(0)
    assert (pp.knn_filter(flipped, k=2, radius=5) - want.flip(0)).abs().max() <= 1e-6
    # pdim = 2: the search ignores the third column, the mean does not
    got = pp.knn_filter(CLOUD, k=1, pdim=2)
    assert (got[2] - torch.tensor([0., 1., 0.5])).abs().max() <= 1e-6 and got.shape == CLOUD.shape
    with pytest.raises(RuntimeError, match="out of range"):
        pp.knn_filter(CLOUD, k=6)

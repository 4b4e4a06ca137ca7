"""pp.nbr_filter / pp.knn_filter with ``_grid=True`` on a host cloud: the grid route needs the kernels, so the tensor route answers."""
import pytest
import torch

import pypose_amd as pp


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_grid_keyword_on_a_host_cloud_is_the_tensor_route(dtype):
    pts = torch.randn(300, 4, generator=torch.Generator().manual_seed(0), dtype=torch.float64).to(dtype)
    for grid in (True, False, None):
        out, mask = pp.nbr_filter(pts, 2, 0.4, pdim=3, return_mask=True, _grid=grid)
        want, wmask = pp.nbr_filter(pts, 2, 0.4, pdim=3, return_mask=True)
        assert not mask.all() and mask.any() and torch.equal(mask, wmask) and torch.equal(out, want)
        assert torch.equal(pp.knn_filter(pts, 3, pdim=3, radius=0.4, _grid=grid), pp.knn_filter(pts, 3, pdim=3, radius=0.4))
        assert torch.equal(pp.knn_filter(pts, 3, pdim=3, _grid=grid), pp.knn_filter(pts, 3, pdim=3))

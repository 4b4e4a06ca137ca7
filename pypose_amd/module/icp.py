"""Iterative closest point (reference pypose/module/icp.py).

On the device (3-D clouds of one dtype, Euclidean distance) one iteration is two launches of csrc/knn.hip and a 3 x 3 SVD: the
partial pass searches the target for every point of ``T . source`` with the cumulative transform ``T`` applied in registers
(the moved cloud is never written), the merge pass leaves ``sum d, sum p, sum q, sum q p^T`` per batch element in fp64, and the
Kabsch step (centroids, centred cross-covariance, SVD, the reflection rule of ``svdtf``) works on those 16 numbers.  Above
``geometry._GRID_ICP_MIN_N2`` target points the search goes through a grid index of the target built once per ``forward``
(csrc/knn_grid.hip): same matches, fewer pairs.  Elsewhere the reference's loop runs over ``pp.knn`` / ``pp.svdtf``.
"""
import torch
from torch import nn

from ..function import geometry as _geo
from ..function.checking import is_SE3
from ..lietensor import SE3, identity_SE3
from ..lietensor.convert import mat2SE3
from ..utils.stepper import ReduceToBason


class ICP(nn.Module):
    """Batched ICP: the rigid transform (``SE3``) that maps ``source (..., N1, 3)`` onto ``target (..., N2, 3)``, alternating
    nearest-neighbour association and the SVD solution of the matched pairs until ``stepper`` (default
    ``ReduceToBason(steps=200)``) stops the loop.  ``init``: the initial ``SE3`` transform (the result depends on it)."""

    def __init__(self, init=None, stepper=None):
        super().__init__()
        self.stepper = ReduceToBason(steps=200) if stepper is None else stepper
        assert init is None or is_SE3(init), "The initial transformation is not SE3Type."
        self.init = init

    def forward(self, source, target, ord=2, dim=-1, init=None):
        init = init if init is not None else self.init
        if init is not None:
            assert is_SE3(init), "The initial transformation is not SE3Type LieTensor."
        if _geo._knn_on_kernels(source, target, 1, ord, dim, False) and (init is None or (init.is_cuda and init.dtype == source.dtype)) \
                and not (torch.is_grad_enabled() and any(t.requires_grad for t in (source, target, init) if t is not None)):
            return self._on_kernels(source, target, init)
        temporal = source if init is None else init.unsqueeze(-2) @ source
        batch = torch.broadcast_shapes(source.shape[:-2], target.shape[:-2])
        self.stepper.reset()
        while self.stepper.continual():
            dist, idx = _geo.knn(temporal, target, k=1, ord=ord, dim=dim)
            error = dist.squeeze(-1).mean(dim=-1)
            target = target.expand(batch + target.shape[-2:])
            matched = torch.gather(target, -2, idx.expand(batch + source.shape[-2:]))
            temporal = _geo.svdtf(temporal, matched).unsqueeze(-2) @ temporal
            self.stepper.step(error)
        return _geo.svdtf(source, temporal)

    def _on_kernels(self, source, target, init):
        lead = [source.shape[:-2], target.shape[:-2]] + ([init.shape[:-1]] if init is not None else [])
        batch = torch.broadcast_shapes(*lead)
        B, n = batch.numel(), source.shape[-2]
        src, ss = _geo._knn_flat(source, batch)
        tgt, ts = _geo._knn_flat(target, batch)
        if init is None:
            T = identity_SE3(B, dtype=source.dtype, device=source.device)
        else:
            T = SE3(init.tensor().expand(batch + (7,)).reshape(B, 7).contiguous())
        ws, grid = {}, None
        if _geo._GRID_ICP_MIN_N2 is not None and target.shape[-2] >= _geo._GRID_ICP_MIN_N2:
            try:        # the target does not move: one index for the whole loop; a rigid motion keeps a compact tile of the source compact
                grid = (_geo.KnnIndex(tgt), _geo._grid_order(src.view(-1, n, 3)))
            except ValueError:                                                        # (non-finite points, the cell cap)
                pass
        self.stepper.reset()
        while self.stepper.continual():
            sums = _geo._icp_stats(src, ss, tgt, ts, T.tensor(), B, ws, grid=grid)
            error = (sums[:, 0] / n).to(source.dtype).view(batch)
            p, q = sums[:, 1:4] / n, sums[:, 4:7] / n
            U, _, Vh = torch.linalg.svd(sums[:, 7:].view(B, 3, 3) - n * q.unsqueeze(-1) * p.unsqueeze(-2))
            R = U @ Vh
            mirrored = (R.det() + 1).abs() < 1e-6
            R[mirrored] = -R[mirrored]
            t = q.unsqueeze(-1) - R @ p.unsqueeze(-1)
            step = mat2SE3(torch.cat((R, t), dim=-1), check=False)
            T = SE3(step.tensor().to(source.dtype)) @ T
            self.stepper.step(error)
        return _geo.svdtf(source, T.lview(*batch).unsqueeze(-2) @ source)

"""EPnP: camera pose from matches of 3-D points and pixels (reference pypose/module/pnp.py; Moreno-Noguer, Lepetit, Fua, IJCV 2009).

On the device (HIP tensors of one dtype, fp32 / fp64, no gradient recorded) the whole batch is ONE launch of csrc/epnp.hip: a
wavefront (N < 256) or a workgroup per problem carries the problem from the control points to the SE3 row, in fp64, without a
global temporary.  Each problem is solved as if alone -- the Gauss-Newton refinement of the betas keeps its own best iterate
instead of stopping on a loss summed over the batch -- and a problem whose points are coplanar, or that meets a non-finite
value, returns a row of NaN (the launch cannot raise without a synchronise).

On host tensors (under the test backend) the tensor formulation below runs: the reference's algorithm on this package's ``svdtf``,
``reprojerr``, ``GaussNewton``, ``LSTSQ`` and ``StopOnPlateau``; differentiable.  Device tensors the kernel does not take (a recorded
gradient, other dtypes) raise: the tensor formulation on the device met a GPU fault inside torch.linalg at B = 64, N = 1024 in fp32
whose cause was not found, so it is not offered there.
"""
import ctypes

import torch
from torch import nn

from .. import _C
from ..function.geometry import cart2homo, reprojerr, svdtf
from ..function.linalg import bmv
from ..lietensor import SE3
from ..optim import GaussNewton
from ..optim.scheduler import StopOnPlateau
from ..optim.solver import LSTSQ

_EPNP_SIG = [ctypes.c_void_p] * 3 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
_REFINE_STEPS = 10
_PAIRS = ((1, 2, 3, 2, 3, 3), (0, 0, 0, 1, 1, 2))                     # the six control-point distances
_QUAD = ((0, 0, 1, 0, 1, 2, 0, 1, 2, 3), (0, 1, 1, 2, 2, 2, 3, 3, 3, 3))   # the ten products beta_a beta_b, in the order of L's columns


class _ControlDistances(nn.Module):
    """residual of Eq. 15: the six distances between the world control points minus those of the camera-frame ones"""

    def __init__(self, beta):
        super().__init__()
        self.beta = nn.Parameter(beta)

    def forward(self, controls, nullv):
        cam = bmv(nullv.mT, self.beta).unflatten(-1, (4, 3))
        i, j = _PAIRS
        return (controls[..., i, :] - controls[..., j, :]).norm(dim=-1) - (cam[..., i, :] - cam[..., j, :]).norm(dim=-1)


def _on_kernels(points, pixels, intrinsics):
    ts = (points, pixels, intrinsics)
    return (_C._test_backend is None and all(t.is_cuda for t in ts) and points.dtype in _C._SUFFIX
            and all(t.dtype == points.dtype and t.device == points.device for t in ts)
            and not (torch.is_grad_enabled() and any(t.requires_grad for t in ts)))


def _launch(points, pixels, intrinsics, steps):
    batch = torch.broadcast_shapes(points.shape[:-2], pixels.shape[:-2], intrinsics.shape[:-2])
    B, N, dt, dev = batch.numel(), points.shape[-2], points.dtype, points.device
    pts = points.expand(batch + (N, 3)).reshape(B, N, 3).contiguous()
    pix = pixels.expand(batch + (N, 2)).reshape(B, N, 2).contiguous()
    if intrinsics.shape[:-2].numel() == 1:          # one matrix for the whole batch: not copied B times
        K, kstride = intrinsics.reshape(3, 3).contiguous(), 0
    else:
        K, kstride = intrinsics.expand(batch + (3, 3)).reshape(B, 3, 3).contiguous(), 9
    pose = torch.empty((B, 7), dtype=dt, device=dev)
    if B:
        name = "pplie_epnp" + _C._SUFFIX[dt]
        with _C._on_device(dev):
            _C.check(_C.library().symbol(name, _EPNP_SIG)(pts.data_ptr(), pix.data_ptr(), K.data_ptr(), kstride, pose.data_ptr(), B, N,
                                                          steps, _C.stream_ptr(dev)), name)
    return SE3(pose.view(batch + (7,)))


class EPnP(nn.Module):
    """Batched EPnP: the camera pose (``SE3``, world -> camera) from ``points (..., N, 3)`` in the world frame and their
    ``pixels (..., N, 2)``, ``N >= 4``, through rectified ``intrinsics (..., 3, 3)`` (given here or per call).  ``refine``:
    Gauss-Newton on the four betas after the closed-form solution."""

    def __init__(self, intrinsics=None, refine=True):
        super().__init__()
        self.refine = refine
        self.solver = LSTSQ()
        if intrinsics is not None:
            self.register_buffer('intrinsics', intrinsics)

    def forward(self, points, pixels, intrinsics=None):
        assert pixels.size(-2) == points.size(-2) >= 4, "Number of points/pixels cannot be smaller than 4."
        intrinsics = self.intrinsics if intrinsics is None else intrinsics
        torch.broadcast_shapes(points.shape[:-2], pixels.shape[:-2], intrinsics.shape[:-2])
        if _on_kernels(points, pixels, intrinsics):
            return _launch(points, pixels, intrinsics, _REFINE_STEPS if self.refine else 0)
        if points.is_cuda and _C._test_backend is None:
            raise NotImplementedError("pypose_amd: EPnP on the device takes fp32 / fp64 tensors of one dtype and device that record no "
                                      "gradient (csrc/epnp.hip); the differentiable tensor formulation runs on host tensors only")
        controls = self._controls(points)
        alpha = torch.linalg.solve(cart2homo(controls), cart2homo(points), left=False)
        nullv = self._null_vectors(pixels, alpha, intrinsics)
        betas = self._betas(*self._l_rho(nullv, controls))
        poses, scales = self._pose(betas, nullv, alpha, points)
        error = reprojerr(points, pixels, intrinsics, poses, reduction='norm').mean(dim=-1, keepdim=True)
        pick = error.argmin(dim=0, keepdim=True)
        pose = poses.gather(0, pick.tile(7)).squeeze(0)
        if self.refine:
            beta = betas.gather(0, pick.tile(4)).squeeze(0) * scales.gather(0, pick).squeeze(0)
            pose, _ = self._pose(self._refine(beta, nullv, controls), nullv, alpha, points)
        return pose

    @staticmethod
    def _controls(points):
        centre = points.mean(dim=-2, keepdim=True)
        spread = points - centre
        _, s, vh = torch.linalg.svd(spread.mT @ spread)
        return torch.cat([centre, centre + s.sqrt().unsqueeze(-1) * vh.mT], dim=-2)

    @staticmethod
    def _null_vectors(pixels, alpha, intrinsics):
        """rows of M (Eq. 7): [alpha_j fu, 0, alpha_j (u0 - u)] and [0, alpha_j fv, alpha_j (v0 - v)]; the eigenvectors of the four
        smallest eigenvalues of M^T M, the smallest last"""
        lead, n = pixels.shape[:-2], pixels.shape[-2]
        focal = torch.stack([intrinsics[..., 0, 0], intrinsics[..., 1, 1]], dim=-1)[..., None, :]
        offset = intrinsics[..., None, :2, 2] - pixels                                         # (u0 - u, v0 - v)
        zero = torch.zeros_like(alpha)
        rows = [torch.stack([alpha * focal[..., 0:1], zero, alpha * offset[..., 0:1]], dim=-1),
                torch.stack([zero, alpha * focal[..., 1:2], alpha * offset[..., 1:2]], dim=-1)]
        M = torch.stack(rows, dim=-3).reshape(*lead, 2 * n, 12)
        w, v = torch.linalg.eig(M.mT @ M)
        w, v = w.real, v.real
        order = w.topk(4, largest=False, sorted=True).indices.flip(-1)
        return torch.gather(v, -1, order.unsqueeze(-2).expand(v.shape[:-1] + (4,))).mT

    @staticmethod
    def _l_rho(nullv, controls):
        i, j = _PAIRS
        a, b = _QUAD
        v = nullv.unflatten(-1, (4, 3))
        dv = v[..., i, :] - v[..., j, :]
        L = (dv[..., a, :, :] * dv[..., b, :, :]).sum(dim=-1).mT
        twice = torch.tensor([1 if x == y else 2 for x, y in zip(a, b)], dtype=L.dtype, device=L.device)
        return L * twice, (controls[..., i, :] - controls[..., j, :]).pow(2).sum(-1)

    def _betas(self, L, rho):
        """the candidates for a null space of dimension 1..4 (Eq. 10-14), ``(4, ..., 4)``"""
        betas = rho.new_zeros((4,) + rho.shape[:-1] + (4,))
        betas[0, ..., 3] = 1
        S = self.solver(L[..., (5, 8, 9)], rho)
        betas[1, ..., 2] = S[..., 0].abs().sqrt()
        betas[1, ..., 3] = S[..., 2].abs().sqrt() * S[..., 1].sign() * S[..., 0].sign()
        S = self.solver(L[..., (2, 4, 7, 5, 8, 9)], rho)
        betas[2, ..., 1] = S[..., 0].abs().sqrt()
        betas[2, ..., 2] = S[..., 3].abs().sqrt() * S[..., 1].sign() * S[..., 0].sign()
        betas[2, ..., 3] = S[..., 5].abs().sqrt() * S[..., 2].sign() * S[..., 0].sign()
        S = self.solver(L, rho)
        betas[3, ..., 0] = S[..., 9].abs().sqrt() * S[..., 6].sign() * S[..., 0].sign()
        betas[3, ..., 1] = S[..., 5].abs().sqrt() * S[..., 3].sign() * S[..., 0].sign()
        betas[3, ..., 2] = S[..., 2].abs().sqrt() * S[..., 1].sign() * S[..., 0].sign()
        betas[3, ..., 3] = S[..., 0].abs().sqrt()
        return betas

    @staticmethod
    def _pose(beta, nullv, alpha, points):
        """camera-frame points of ``beta``, scaled to the spread of the world cloud and flipped in front of the camera, and the
        rigid transform onto them; returns (pose, signed scale ``(..., 1)``)"""
        controls = bmv(nullv.mT, beta).unflatten(-1, (4, 3))
        cam = alpha @ controls
        dw = (points - points.mean(dim=-2, keepdim=True)).norm(dim=-1)
        dc = (cam - cam.mean(dim=-2, keepdim=True)).norm(dim=-1)
        scale = torch.linalg.vecdot(dc, dw) / torch.linalg.vecdot(dc, dc)
        cam = alpha @ (controls * scale[..., None, None])
        sign = 1 - 2 * torch.any(cam[..., 2] < 0, dim=-1).to(scale.dtype)
        return svdtf(points, sign[..., None, None] * cam), (sign * scale).unsqueeze(-1)

    @staticmethod
    def _refine(beta, nullv, controls):
        model = _ControlDistances(beta)
        StopOnPlateau(GaussNewton(model, solver=LSTSQ()), steps=_REFINE_STEPS, patience=3).optimize(input=(controls, nullv))
        return beta + (model.beta - beta).detach()          # the gradient of the initial beta survives the optimisation

"""Camera geometry either side of the bundle-adjustment path.

Host-side mirror of the five pinhole helpers of pypose/function/geometry.py (cart2homo :8, homo2cart :37,
point2pixel :60, pixel2point :115, reprojerr :171): same names, argument meaning, broadcasting and assertion
messages.  With extrinsics, ``point2pixel`` / ``reprojerr`` are ONE kernel per direction (csrc/reproj.hip): the forward
``pplie_se3_reproj_lin`` returns the residual together with its closed-form Jacobian blocks [d r/d pose | d r/d point],
the backward ``pplie_reproj_vjp`` contracts them -- and the LM optimizers take the blocks as they are instead of
sweeping the autograd graph (``closed_form_blocks`` below, optim/multigraph.py).  Without extrinsics the pinhole
algebra is plain tensor arithmetic on whatever device the inputs live on.

``bal_point2pixel`` / ``bal_reprojerr`` are the Snavely / BAL model of the reference's bundle-adjustment example (focal length
and two radial distortion coefficients per camera) the same way (csrc/bal.hip): ``pplie_se3_bal_lin`` returns the residual and
the blocks for intrinsics, pose and point, ``pplie_bal_vjp`` contracts all three.

``knn`` (reference geometry.py:228-313) streams the neighbour cloud through LDS and keeps every reference point's best k in
registers (csrc/knn.hip): the ``[N1, N2]`` distance matrix of the reference formulation is never formed.  ``_icp_stats`` is the
same pass with the sums one ICP iteration needs (module/icp.py).  ``knn_index`` builds a uniform grid over a neighbour cloud once
(csrc/knn_grid.hip); ``knn(ref, index)`` then searches only the cells around every query, with the same results bit for bit.

``nbr_filter`` / ``knn_filter`` / ``voxel_filter`` (reference geometry.py:436-664) are the steps before registration
(csrc/cloud_filter.hip): the cloud streamed against itself with a count under the radius kept next to the best-k list, and voxel
keys plus a segmented mean over the sorted keys; on large clouds the two neighbour filters search through the grid index instead
(csrc/nbr_grid.hip: only the cells within the radius).  ``random_filter`` is an index.
"""
import ctypes
import math

import torch

from .. import _C
from ..lietensor import LieTensor
from ..lietensor import operation as _op

_ReprojVjp = _op._make_bwd("ReprojVjp", "reproj_vjp", (18, 2), (7, 3))
_closed_recorders = []          # optim: active recorders of (residual, inputs, closed-form blocks)


class _Reproj(torch.autograd.Function):
    """r = homo2cart(K (X . p)) - pixel for broadcastable (pose [...,7], point [...,3], cam [...,11]); saves J [...,18]."""

    @staticmethod
    def forward(X, p, cam):
        r, J = _op._launch("se3_reproj_lin", (X, p, cam), (7, 3, 11), (2, 18))
        return r, J

    @staticmethod
    def setup_context(ctx, inputs, output):
        ctx.save_for_backward(*inputs, output[1])
        ctx.mark_non_differentiable(output[1])
        ctx.shapes = [tuple(t.shape) for t in inputs]

    @staticmethod
    def backward(ctx, g, _gJ):
        X, p, cam, J = ctx.saved_tensors
        gX, gp = _ReprojVjp.apply(J, g)
        gcam = None
        if ctx.needs_input_grad[2]:
            # intrinsics / observed pixel (rarely optimised): d r/d K = (d pix/d h) (x) q, d r/d pixel = -I
            q = _op._launch("se3_act_fwd", (X, p), (7, 3), (3,))[0]
            K = cam[..., :9].reshape(cam.shape[:-1] + (3, 3))
            h = (K @ q.unsqueeze(-1)).squeeze(-1)
            hz = h[..., 2:]
            tiny = torch.finfo(h.dtype).tiny
            clamped = hz.abs() < tiny
            den = torch.where(hz < 0, -torch.ones_like(hz), torch.ones_like(hz)) * hz.abs().clamp(min=tiny)
            pix = h[..., :2] / den
            gh = torch.cat([g / den, -(pix * g).sum(-1, keepdim=True) / den * (~clamped)], -1)
            gcam = torch.cat([(gh.unsqueeze(-1) * q.unsqueeze(-2)).reshape(gh.shape[:-1] + (9,)), -g], -1)
        out = []
        for grad, shape in zip((gX, gp, gcam), ctx.shapes):
            out.append(None if grad is None else grad.sum_to_size(shape) if tuple(grad.shape) != shape else grad)
        return tuple(out)

    @staticmethod
    def vmap(info, in_dims, X, p, cam):
        X, p, cam = _op._fold_vmap(in_dims, (X, p, cam))
        return _Reproj.apply(X, p, cam), (0, 0)


def _reproject(points, intrinsics, extrinsics, pixels):
    """(..., N, 2) residual through the fused kernels; the closed-form blocks are offered to an active optimizer trace."""
    X = extrinsics.tensor().unsqueeze(-2)                                           # (..., 1, 7): one pose, N points
    K9 = intrinsics.reshape(intrinsics.shape[:-2] + (1, 9))
    lead = torch.broadcast_shapes(points.shape[:-1], X.shape[:-1], K9.shape[:-1], pixels.shape[:-1] if pixels is not None else ())
    uv = pixels if pixels is not None else points.new_zeros(lead + (2,))
    cam = torch.cat([K9.expand(lead + (9,)).to(points.dtype), uv.expand(lead + (2,))], -1)
    r, J = _Reproj.apply(X, points, cam)
    if _closed_recorders:
        Jm = J.reshape(J.shape[:-1] + (2, 9))
        for rec in _closed_recorders:
            rec.note_closed(r, [(extrinsics, Jm[..., :6]), (points, Jm[..., 6:9])],
                            blockers=[t for t in (intrinsics, pixels) if t is not None and t.requires_grad])
    return r


# ---- Snavely / BAL model (csrc/bal.hip): four operands in, three gradients out -- entry points with explicit pointer
# arguments, launched from here (the uniform row launcher _C.row_op carries 3 inputs and 2 outputs)
_BAL_FWD_SIG = [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_void_p]
_BAL_LIN_SIG = [ctypes.c_void_p] * 6 + [ctypes.c_int64, ctypes.c_void_p]
_BAL_VJP_SIG = [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_void_p]


def _bal_call(name, sig, ins, in_widths, out_widths):
    """``pplie_<name>_{f32,f64}`` on contiguous ``[n, w]`` device tensors (a ``None`` input is a NULL pointer); returns the
    freshly allocated outputs"""
    x0 = ins[0]
    n = x0.shape[0]
    for t, w in zip(ins, in_widths):
        if t is not None and (t.dim() != 2 or t.shape != (n, w) or t.dtype != x0.dtype or t.device != x0.device
                              or not t.is_contiguous() or not t.is_cuda):
            raise ValueError(f"pypose_amd: {name}: inputs must be contiguous [N,W] device tensors of one dtype")
    if x0.dtype not in _C._SUFFIX:
        raise TypeError(f"pypose_amd: {name} supports float32/float64, got {x0.dtype}")
    outs = tuple(torch.empty((n, w), dtype=x0.dtype, device=x0.device) for w in out_widths)
    if n:
        sym = "pplie_" + name + _C._SUFFIX[x0.dtype]
        fn = _C.library().symbol(sym, sig)
        with _C._on_device(x0.device):
            code = fn(*[None if t is None else t.data_ptr() for t in ins], *[o.data_ptr() for o in outs], n, _C.stream_ptr(x0.device))
        _C.check(code, sym)
    return outs


def _bal_fwd(K, X, p, uv=None):
    return _bal_call("se3_bal_fwd", _BAL_FWD_SIG, (K, X, p, uv), (3, 7, 3, 2), (2,))[0]


def _bal_lin(K, X, p, uv=None):
    return _bal_call("se3_bal_lin", _BAL_LIN_SIG, (K, X, p, uv), (3, 7, 3, 2), (2, 24))


def _bal_vjp(J, g):
    return _bal_call("bal_vjp", _BAL_VJP_SIG, (J, g), (24, 2), (3, 7, 3))


def _bal_rows(t, lead, w):
    """``t`` broadcast to ``lead + (w,)`` as contiguous rows; an already contiguous operand of that shape is not copied"""
    if t is None:
        return None
    if t.shape[:-1] != lead:
        t = t.expand(lead + (w,))
    return t.reshape(-1, w).contiguous()


def _bal_composed(K, X, p, uv):
    """the model from the differentiable ops (SE3 Act + tensor arithmetic): host tensors, other dtypes, a stand-in back end,
    and the backward of the backward"""
    from ..lietensor import lietensor as lt
    q = (X if isinstance(X, LieTensor) else lt._wrap(X, lt.SE3_type)).Act(p)
    n = -q[..., :2] / q[..., 2:3]
    rho = n.square().sum(dim=-1, keepdim=True)
    u = K[..., :1] * (1 + K[..., 1:2] * rho + K[..., 2:3] * rho.square()) * n
    return u if uv is None else u - uv


class _BalVjp(torch.autograd.Function):
    """(gK, gX, gp) = g J in one launch (``pplie_bal_vjp``); J [..., 24] is shared by every slice of a batched cotangent"""

    @staticmethod
    def forward(J, g):
        if _op._is_legacy_batched(g):
            # jacobian(vectorize=True) / the optimizers' block sweeps: the legacy vmap does not consult Function.vmap
            lvl = _op._legacy_level(g)
            gb = torch._remove_batch_dim(g, lvl, 1, 0)
            outs = [_BalVjp.forward(J, gb[b]) for b in range(gb.shape[0])]
            return tuple(torch._add_batch_dim(torch.stack([o[k] for o in outs]), 0, lvl) for k in range(3))
        lead = J.shape[:-1]
        outs = _bal_vjp(J.reshape(-1, 24), _bal_rows(g, lead, 2))
        return tuple(o.view(lead + (w,)) for o, w in zip(outs, (3, 7, 3)))

    @staticmethod
    def setup_context(ctx, inputs, output):
        pass

    @staticmethod
    def backward(ctx, *grads):
        raise NotImplementedError("BalVjp: a recorded backward takes the composed route (_BalReproj.backward)")

    @staticmethod
    def vmap(info, in_dims, J, g):
        J, g = _op._fold_vmap(in_dims, (J, g))
        return _BalVjp.apply(J.contiguous(), g), (0, 0, 0)


class _BalReproj(torch.autograd.Function):
    """r = f (1 + k1 |n|^2 + k2 |n|^4) n - uv, n = -q_xy / q_z, q = X . p, for broadcastable (K [...,3], pose [...,7],
    point [...,3], uv [...,2] or None); saves J [...,24] = 2 x [dK | dpose | dpoint]."""

    @staticmethod
    def forward(K, X, p, uv):
        lead = torch.broadcast_shapes(*[t.shape[:-1] for t in (K, X, p, uv) if t is not None])
        r, J = _bal_lin(_bal_rows(K, lead, 3), _bal_rows(X, lead, 7), _bal_rows(p, lead, 3), _bal_rows(uv, lead, 2))
        return r.view(lead + (2,)), J.view(lead + (24,))

    @staticmethod
    def setup_context(ctx, inputs, output):
        ctx.save_for_backward(output[1], *[t for t in inputs if t is not None])
        ctx.mark_non_differentiable(output[1])
        ctx.has_uv = inputs[3] is not None
        ctx.shapes = [None if t is None else tuple(t.shape) for t in inputs]

    @staticmethod
    def backward(ctx, g, _gJ):
        J, K, X, p, *uv = ctx.saved_tensors
        if torch.is_grad_enabled():
            # the backward itself is being recorded (create_graph=True): the same gradients from differentiable ops
            ins = [t if t.requires_grad else t.detach().requires_grad_(True) for t in (K, X, p, *uv)]
            out = _bal_composed(ins[0], ins[1], ins[2], ins[3] if uv else None)
            grads = list(torch.autograd.grad([out], ins, [g.expand_as(out)], create_graph=True, allow_unused=True))
            if not uv:
                grads.append(None)
        else:
            gK, gX, gp = _BalVjp.apply(J, g)
            grads = [gK, gX, gp, -g if ctx.has_uv and ctx.needs_input_grad[3] else None]
        out = []
        for grad, shape in zip(grads, ctx.shapes):
            out.append(None if grad is None or shape is None else grad.sum_to_size(shape) if tuple(grad.shape) != shape else grad)
        return tuple(out)

    @staticmethod
    def vmap(info, in_dims, K, X, p, uv):
        if uv is None:
            K, X, p = _op._fold_vmap(in_dims[:3], (K, X, p))
        else:
            K, X, p, uv = _op._fold_vmap(in_dims, (K, X, p, uv))
        return _BalReproj.apply(K, X, p, uv), (0, 0)


def _bal_on_kernels(*tensors):
    t0 = tensors[0]
    return _C._test_backend is None and all(t.is_cuda and t.dtype == t0.dtype for t in tensors) \
        and t0.dtype in (torch.float32, torch.float64)


def _bal_project(points, intrinsics, extrinsics, pixels):
    """(..., 2) BAL residual (projection when ``pixels`` is None) through csrc/bal.hip; the closed-form blocks of all three
    operands are offered to an active optimizer trace"""
    present = [t for t in (intrinsics, extrinsics, points, pixels) if t is not None]
    if not _bal_on_kernels(*present):
        return _bal_composed(intrinsics, extrinsics, points, pixels)
    X = extrinsics.tensor()
    if not _closed_recorders and not (torch.is_grad_enabled() and any(t.requires_grad for t in present)) \
            and not torch._C._are_functorch_transforms_active():
        lead = torch.broadcast_shapes(*[t.shape[:-1] for t in present])
        r = _bal_fwd(_bal_rows(intrinsics, lead, 3), _bal_rows(X, lead, 7), _bal_rows(points, lead, 3), _bal_rows(pixels, lead, 2))
        return r.view(lead + (2,))
    r, J = _BalReproj.apply(intrinsics, X, points, pixels)
    if _closed_recorders:
        Jm = J.reshape(J.shape[:-1] + (2, 12))
        for rec in _closed_recorders:
            rec.note_closed(r, [(intrinsics, Jm[..., 0:3]), (extrinsics, Jm[..., 3:9]), (points, Jm[..., 9:12])],
                            blockers=[pixels] if pixels is not None and pixels.requires_grad else [])
    return r


def _need(cond, msg):
    assert cond, msg


def _is_k(intrinsics):
    return intrinsics.shape[-2:] == (3, 3)


def cart2homo(coordinates):
    """``(*, D) -> (*, D + 1)``: append a one."""
    return torch.cat([coordinates, coordinates.new_ones(coordinates.shape[:-1] + (1,))], dim=-1)


def homo2cart(coordinates):
    """``(*, D + 1) -> (*, D)``: divide by the last component; a zero (of either sign) is replaced by the
    smallest normal number with the sign convention ``pm(0) = +1`` of the reference."""
    w = coordinates[..., -1:]
    tiny = torch.finfo(coordinates.dtype).tiny
    sign = torch.where(w < 0, -torch.ones_like(w), torch.ones_like(w))
    return coordinates[..., :-1] / (sign * w.abs().clamp(min=tiny))


def point2pixel(points, intrinsics, extrinsics=None):
    """Pixels ``(*, N, 2)`` of ``points (*, N, 3)`` seen through ``intrinsics (*, 3, 3)``; with ``extrinsics``
    (SE3 ``(*, 7)``, world -> camera) the points are transformed first."""
    _need(points.size(-1) == 3, "Points shape incorrect")
    _need(_is_k(intrinsics), "Intrinsics shape incorrect.")
    lead = [points.shape[:-2], intrinsics.shape[:-2]]
    if extrinsics is not None:
        _need(isinstance(extrinsics, LieTensor) and extrinsics.shape[-1] == 7, "Type incorrect.")
        lead.append(extrinsics.shape[:-1])
    torch.broadcast_shapes(*lead)                                      # raises on incompatible batch dims
    if extrinsics is not None:
        return _reproject(points, intrinsics, extrinsics, None)
    return homo2cart(points @ intrinsics.mT)


def pixel2point(pixels, depth, intrinsics):
    """Camera-frame points ``(*, N, 3)`` of ``pixels (*, N, 2)`` at ``depth (*, N)``."""
    _need(pixels.size(-1) == 2, "Pixels shape incorrect")
    _need(depth.size(-1) == pixels.size(-2), "Depth shape does not match pixels")
    _need(_is_k(intrinsics), "Intrinsics shape incorrect.")
    focal = torch.stack([intrinsics[..., 0, 0], intrinsics[..., 1, 1]], dim=-1)
    centre = torch.stack([intrinsics[..., 0, 2], intrinsics[..., 1, 2]], dim=-1)
    _need(not torch.any(focal[..., 0] == 0), "fx Cannot contain zero")
    _need(not torch.any(focal[..., 1] == 0), "fy Cannot contain zero")
    xy = (pixels - centre.unsqueeze(-2)) * depth.unsqueeze(-1) / focal.unsqueeze(-2)
    return torch.cat([xy, depth.unsqueeze(-1)], dim=-1)


def reprojerr(points, pixels, intrinsics, extrinsics=None, reduction='none'):
    """Projected minus observed pixels: ``'none'`` -> ``(*, N, 2)``; ``'norm'`` / ``'sum'`` reduce the last dim."""
    torch.broadcast_shapes(points.shape[:-2], pixels.shape[:-2], intrinsics.shape[:-2])
    _need(points.size(-1) == 3 and pixels.size(-1) == 2 and _is_k(intrinsics), "Shape not compatible.")
    _need(reduction in {'norm', 'sum', 'none'}, "Reduction method can only be 'norm'|'sum'|'none'.")
    if extrinsics is not None:
        _need(isinstance(extrinsics, LieTensor) and extrinsics.shape[-1] == 7, "Type incorrect.")
        torch.broadcast_shapes(points.shape[:-2], intrinsics.shape[:-2], extrinsics.shape[:-1])
        err = _reproject(points, intrinsics, extrinsics, pixels)
    else:
        err = point2pixel(points, intrinsics) - pixels
    return {'none': lambda e: e, 'norm': lambda e: e.norm(dim=-1), 'sum': lambda e: e.sum(dim=-1)}[reduction](err)


def _bal_check(points, intrinsics, extrinsics, pixels=None):
    _need(points.size(-1) == 3, "Points shape incorrect")
    _need(intrinsics.size(-1) == 3, "Intrinsics shape incorrect.")
    _need(isinstance(extrinsics, LieTensor) and extrinsics.shape[-1] == 7, "Type incorrect.")
    lead = [points.shape[:-1], intrinsics.shape[:-1], extrinsics.shape[:-1]]
    if pixels is not None:
        _need(pixels.size(-1) == 2, "Shape not compatible.")
        lead.append(pixels.shape[:-1])
    torch.broadcast_shapes(*lead)                                      # raises on incompatible batch dims


def bal_point2pixel(points, intrinsics, extrinsics):
    """Pixels ``(*, 2)`` of ``points (*, 3)`` through the Snavely / BAL camera model: ``q = extrinsics . points``,
    ``n = -q[:2] / q[2]``, ``u = f (1 + k1 |n|^2 + k2 |n|^4) n`` with ``intrinsics (*, 3) = (f, k1, k2)`` and ``extrinsics``
    an SE3 ``(*, 7)``, world -> camera.  The leading dimensions broadcast.  One kernel on the device (csrc/bal.hip)."""
    _bal_check(points, intrinsics, extrinsics)
    return _bal_project(points, intrinsics, extrinsics, None)


def bal_reprojerr(points, pixels, intrinsics, extrinsics, reduction='none'):
    """:func:`bal_point2pixel` minus the observed ``pixels (*, 2)``: ``'none'`` -> ``(*, 2)``; ``'norm'`` / ``'sum'`` reduce
    the last dim.  The kernel returns the residual together with its closed-form Jacobian blocks with respect to the
    intrinsics, the pose and the point; the backward contracts them in one launch and the LM optimizers take them as they
    are instead of sweeping the autograd graph."""
    _bal_check(points, intrinsics, extrinsics, pixels)
    _need(reduction in {'norm', 'sum', 'none'}, "Reduction method can only be 'norm'|'sum'|'none'.")
    err = _bal_project(points, intrinsics, extrinsics, pixels)
    return {'none': lambda e: e, 'norm': lambda e: e.norm(dim=-1), 'sum': lambda e: e.sum(dim=-1)}[reduction](err)


# ---- nearest neighbours and ICP correspondences (csrc/knn.hip)
_KNN_BLOCK, _KNN_TILE, _KNN_MAXK = 256, 1024, 16
_KNN_PARTIAL_SIG = [ctypes.c_void_p] * 7 + [ctypes.c_int64] * 3 + [ctypes.c_int] * 2 + [ctypes.c_int64] * 2 + [ctypes.c_void_p]
_KNN_MERGE_SIG = [ctypes.c_void_p] * 10 + [ctypes.c_int64] * 3 + [ctypes.c_int] * 2 + [ctypes.c_int64] * 2 + [ctypes.c_void_p]
_KNN_CHUNK = 1 << 24          # elements of the tensor formulation's [chunk, N2, D] temporary


def _knn_on_kernels(ref, nbr, k, ord, dim, largest):
    """the kernels take 3-D HIP clouds of one dtype (fp32 / fp64), the Euclidean norm over the last dimension and the
    k <= 16 smallest; everything else is the tensor formulation's"""
    return (_C._test_backend is None and ref.is_cuda and nbr.is_cuda and ref.device == nbr.device and ref.dtype == nbr.dtype
            and ref.dtype in _C._SUFFIX and ref.dim() >= 2 and nbr.dim() >= 2 and ref.shape[-1] == 3 and nbr.shape[-1] == 3
            and ord == 2 and dim == -1 and not largest and 1 <= k <= _KNN_MAXK and ref.shape[-2] > 0
            and 0 < nbr.shape[-2] < 2 ** 31 and ref.shape[-2] < 2 ** 31
            and 0 < torch.broadcast_shapes(ref.shape[:-2], nbr.shape[:-2]).numel() <= 65535)


def _knn_flat(t, batch):
    """``t [..., N, 3]`` as contiguous rows and its batch stride in points: a cloud shared by the whole batch is not copied
    (stride 0)"""
    n = t.shape[-2]
    if t.shape[:-2].numel() == 1:
        return t.reshape(n, 3).contiguous(), 0
    return t.expand(batch + (n, 3)).reshape(-1, n, 3).contiguous(), n


def _knn_launch(ref, rs, nbr, ns, B, k, T=None, splits=None, stats=None, grid=None):
    """partial pass (+ merge pass) on flattened clouds.  Returns (values, indices) ``[B, N1, k]``, or with ``stats`` (a dict
    that keeps the scratch of an ICP loop between iterations) the 16 fp64 sums ``[B, 16]`` of the k = 1 correspondences.
    With ``grid = (KnnIndex of nbr, query order or None)`` the partial lists come from the grid query (one split)."""
    N1, N2, dev, dt = ref.shape[-2], nbr.shape[-2], ref.device, ref.dtype
    nt = -(-N2 // _KNN_TILE)
    S = splits if splits is not None else -(-512 // (B * -(-N1 // _KNN_BLOCK)))       # about two workgroups per CU
    S = 1 if grid is not None else max(1, min(S, nt))
    lib, sfx = _C.library(), _C._SUFFIX[dt]
    partial = lib.symbol("pplie_knn_partial" + sfx, _KNN_PARTIAL_SIG)
    merge = lib.symbol("pplie_knn_merge" + sfx, _KNN_MERGE_SIG)
    tp = None if T is None else T.data_ptr()
    with _C._on_device(dev):
        st = _C.stream_ptr(dev)
        if stats is None:
            values = torch.empty((B, N1, k), dtype=dt, device=dev)
            indices = torch.empty((B, N1, k), dtype=torch.int64, device=dev)
            if S == 1 and grid is None:
                _C.check(partial(ref.data_ptr(), nbr.data_ptr(), tp, None, None, values.data_ptr(), indices.data_ptr(), B, N1, N2, k, 1,
                                 rs, ns, st), "pplie_knn_partial" + sfx)
                return values, indices
        key = (B, S, N1, k, dt, dev)
        if stats is None or stats.get("key") != key:
            ws = {"key": key, "pd2": torch.empty((B, S, N1, k), dtype=dt, device=dev),
                  "pidx": torch.empty((B, S, N1, k), dtype=torch.int32, device=dev)}
            if stats is not None:
                ws.update(wg=torch.empty((B, -(-N1 // _KNN_BLOCK), 16), dtype=torch.float64, device=dev),
                          cnt=torch.zeros(B, dtype=torch.int32, device=dev))        # the kernel leaves the counters zero
                stats.clear()
                stats.update(ws)
        else:
            ws = stats
        if grid is None:
            _C.check(partial(ref.data_ptr(), nbr.data_ptr(), tp, ws["pd2"].data_ptr(), ws["pidx"].data_ptr(), None, None, B, N1, N2, k, S,
                             rs, ns, st), "pplie_knn_partial" + sfx)
        else:
            index, order = grid
            _C.check(lib.symbol("pplie_knn_grid" + sfx, _GRID_QUERY_SIG)(
                ref.data_ptr(), tp, None if order is None else order.data_ptr(), index.planes.data_ptr(), index.oidx.data_ptr(),
                index.starts.data_ptr(), index.header.data_ptr(), index.cbase.data_ptr(), ws["pd2"].data_ptr(), ws["pidx"].data_ptr(),
                B, N1, index.planes.shape[1], k, rs, rs, 1 if ns else 0, st), "pplie_knn_grid" + sfx)
        if stats is None:
            _C.check(merge(ws["pd2"].data_ptr(), ws["pidx"].data_ptr(), values.data_ptr(), indices.data_ptr(), None, None, None, None,
                           None, None, B, N1, N2, k, S, rs, ns, st), "pplie_knn_merge" + sfx)
            return values, indices
        sums = torch.empty((B, 16), dtype=torch.float64, device=dev)
        _C.check(merge(ws["pd2"].data_ptr(), ws["pidx"].data_ptr(), None, None, ref.data_ptr(), nbr.data_ptr(), tp, ws["wg"].data_ptr(),
                       ws["cnt"].data_ptr(), sums.data_ptr(), B, N1, N2, 1, S, rs, ns, st), "pplie_knn_merge" + sfx)
        return sums


def _icp_stats(source, ss, target, ts, T, B, ws, splits=None, grid=None):
    """per batch element, over the nearest target point q of every p = T . source: ``[sum d, sum p (3), sum q (3),
    sum q p^T (9)]`` in fp64 ``[B, 16]`` -- two launches, the moved cloud is never written.  ``grid``: (the target's KnnIndex,
    the order of the source or None) searches the index instead of the whole target."""
    return _knn_launch(source, ss, target, ts, B, 1, T=T, splits=splits, stats=ws, grid=grid)


# ---- exact nearest neighbours through a uniform grid over the neighbour cloud (csrc/knn_grid.hip)
_GRID_OCCUPANCY = 8.0         # mean points per cell of the bounding box (swept 4 / 8 / 16)
_GRID_ORDER_OCCUPANCY = 256.0  # ... of the coarse grid the queries are ordered by: about one workgroup per cell
_GRID_MAX_CELLS = 1 << 24
_GRID_KNN_MIN = (1_000_000, 1_000_000)   # (N1, N2) from which pp.knn(ref, tensor) builds an index itself (measured, section 3.9)
_GRID_ICP_MIN_N2 = None       # N2 from which ICP builds the index of its target; None: off (the grid lost at 1e4 x 1e5)
# N from which nbr_filter (count only) / knn_filter (lists) build an index of the cloud themselves, unless the radius's cell box
# is estimated to hold more than the share of the cloud below (_filter_index; measured); None: off
_GRID_FILTER_MIN_N = (100_000, 1_000_000)
_GRID_FILTER_BOX_SHARE = 1 / 128
_NBR_GRID_SIG = [ctypes.c_void_p] * 6 + [ctypes.c_double, ctypes.c_int] + [ctypes.c_int64] * 2 + [ctypes.c_void_p]
_GRID_BBOX_SIG =[ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_double] + [ctypes.c_void_p] * 3
_GRID_KEYS_SIG = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_void_p] * 4
_GRID_TABLES_SIG = [ctypes.c_void_p] * 3 + [ctypes.c_int64] * 3 + [ctypes.c_void_p] * 4
_GRID_QUERY_SIG = [ctypes.c_void_p] * 10 + [ctypes.c_int64] * 3 + [ctypes.c_int] + [ctypes.c_int64] * 2 + [ctypes.c_int, ctypes.c_void_p]


def _grid_keys(flat, occupancy, cells=None):
    """header ``[B, 8]`` (fp64: min, h, gx, gy, gz, non-finite flag) and int32 cell keys ``[B * N]`` of ``flat [B, N, 3]``.
    ``cells(header)`` returns the first cell of every batch element (int32 ``[B]``, on the device); without it the elements
    are 2^21 cells apart."""
    B, N = flat.shape[:2]
    dev, lib, sfx = flat.device, _C.library(), _C._SUFFIX[flat.dtype]
    part = torch.empty((B, min(256, -(-N // 256)), 7), dtype=flat.dtype, device=dev)
    header = torch.empty((B, 8), dtype=torch.float64, device=dev)
    keys = torch.empty(B * N, dtype=torch.int32, device=dev)
    st = _C.stream_ptr(dev)
    _C.check(lib.symbol("pplie_knn_grid_bbox" + sfx, _GRID_BBOX_SIG)(flat.data_ptr(), B, N, occupancy, part.data_ptr(), header.data_ptr(),
                                                                     st), "pplie_knn_grid_bbox" + sfx)
    cbase = None if cells is None else cells(header)
    _C.check(lib.symbol("pplie_knn_grid_keys" + sfx, _GRID_KEYS_SIG)(flat.data_ptr(), B, N, header.data_ptr(),
                                                                     None if cbase is None else cbase.data_ptr(), keys.data_ptr(), st),
             "pplie_knn_grid_keys" + sfx)
    return header, cbase, keys


def _grid_order(flat):
    """the order in which the grid query takes the points of ``flat [B, N, 3]`` (a locality hint: neighbours in the list are
    neighbours in space, so a workgroup's 256 queries share a small cell box), or None where it would not help"""
    if flat.shape[1] <= _KNN_BLOCK or flat.shape[0] > 1023:
        return None
    with _C._on_device(flat.device):
        return torch.sort(_grid_keys(flat, _GRID_ORDER_OCCUPANCY)[2], stable=True).indices


class KnnIndex:
    """A uniform grid over the cloud ``nbr (..., N2, 3)`` for :func:`knn`: the cloud sorted by cell as three planes, the
    permutation back to the original indices and the table of cell starts (csrc/knn_grid.hip).  Built once by
    :func:`knn_index`, searched many times; the results are the brute-force route's bit for bit."""

    def __init__(self, nbr, occupancy=_GRID_OCCUPANCY):
        why = None
        if not (isinstance(nbr, torch.Tensor) and nbr.is_cuda and _C._test_backend is None):
            why = "the cloud is not on a HIP device"
        elif nbr.dtype not in _C._SUFFIX:
            why = f"dtype {nbr.dtype} (float32 / float64 only)"
        elif nbr.dim() < 2 or nbr.shape[-1] != 3:
            why = f"shape {tuple(nbr.shape)} (the points must be 3-D: (..., N2, 3))"
        elif nbr.numel() == 0:
            why = "the cloud is empty"
        elif nbr.shape[:-2].numel() > 65535 or nbr.numel() // 3 > 2 ** 30:
            why = "more than 65535 clouds or 2^30 points"
        if why is not None:
            raise ValueError("pypose_amd: knn_index: " + why)
        self.cloud, self.batch, self.n2, self.occupancy = nbr, nbr.shape[:-2], nbr.shape[-2], float(occupancy)
        B, N = self.batch.numel(), self.n2
        flat = nbr.detach().reshape(B, N, 3).contiguous()
        self.flat, self.ns = (flat[0], 0) if B == 1 else (flat, N)        # as _knn_flat gives a cloud
        dev, sfx = nbr.device, _C._SUFFIX[nbr.dtype]

        def cells(header):                                                # the one host read: sizes and flags
            host = self.header_host = header.cpu()
            if host[:, 7].any():
                raise ValueError("pypose_amd: knn_index: the cloud has non-finite points")
            count = host[:, 4:7].prod(dim=1).to(torch.int64)
            self.cells = int(count.sum())
            if self.cells > _GRID_MAX_CELLS:
                raise ValueError(f"pypose_amd: knn_index: {self.cells} cells for {B} clouds (at most 2^24)")
            return (torch.cumsum(count, 0) - count).to(torch.int32).to(dev)

        with _C._on_device(dev):
            self.header, self.cbase, keys = _grid_keys(flat, self.occupancy, cells)
            keys, self.perm = torch.sort(keys, stable=True)                 # (kept: the cloud's own order as queries, nbr_grid)
            perm = self.perm
            self.planes = torch.empty((3, B * N), dtype=nbr.dtype, device=dev)
            self.oidx = torch.empty(B * N, dtype=torch.int32, device=dev)
            self.starts = torch.empty(self.cells + 1, dtype=torch.int32, device=dev)
            _C.check(_C.library().symbol("pplie_knn_grid_tables" + sfx, _GRID_TABLES_SIG)(
                flat.data_ptr(), keys.data_ptr(), perm.data_ptr(), B, N, self.cells, self.planes.data_ptr(), self.oidx.data_ptr(),
                self.starts.data_ptr(), _C.stream_ptr(dev)), "pplie_knn_grid_tables" + sfx)


def knn_index(nbr, _occupancy=_GRID_OCCUPANCY):
    """The :class:`KnnIndex` of ``nbr (..., N2, 3)``, to be passed to :func:`knn` in the place of the cloud.  Raises
    ``ValueError`` with the reason for anything the grid kernels do not take: a cloud that is not on a HIP device, not float32 /
    float64, not 3-D, empty, with non-finite points, or a batch whose grids need more than 2^24 cells."""
    return KnnIndex(nbr, _occupancy)


def _knn_tensor(ref, nbr, k, ord, dim, largest, sorted):
    """the reference's formulation, norm(ref[..., :, None, :] - nbr[..., None, :, :]).topk, in chunks of reference points so
    that the temporary stays bounded (any device, width, norm and dtype; ``largest``; k > 16)"""
    def one(r):
        return torch.linalg.norm(r.unsqueeze(-2) - nbr.unsqueeze(-3), dim=dim, ord=ord).topk(k, dim=dim, largest=largest, sorted=sorted)
    n1 = ref.shape[-2]
    lead = torch.broadcast_shapes(ref.shape[:-2], nbr.shape[:-2]).numel()
    chunk = max(1, _KNN_CHUNK // max(1, lead * nbr.shape[-2] * max(ref.shape[-1], nbr.shape[-1])))
    if dim != -1 or n1 <= chunk:
        return one(ref)
    parts = [one(ref[..., i:i + chunk, :]) for i in range(0, n1, chunk)]
    return torch.return_types.topk((torch.cat([p.values for p in parts], -2), torch.cat([p.indices for p in parts], -2)))


def knn(ref, nbr, k=1, ord=2, dim=-1, largest=False, sorted=True, _splits=None, _order=True):
    """The ``k`` nearest (``largest``: furthest) points of ``nbr (..., N2, D)`` for every point of ``ref (..., N1, D)`` in the
    ``ord``-norm: ``torch.return_types.topk(values, indices)``, both ``(..., N1, k)`` (reference geometry.py:228-313).

    3-D clouds of one dtype (fp32 / fp64) on the device with ``ord=2, dim=-1, largest=False, k <= 16`` run in csrc/knn.hip: the
    neighbour cloud is streamed through LDS, every reference point keeps its best k in registers, and the ``[N1, N2]``
    distance matrix is never formed; equal distances go to the smaller index.  Everything else takes the tensor formulation.
    When a gradient is recorded the indices come from the kernels and the values are recomputed from the gathered
    neighbours, which gives the reference's gradients in O(N1 k) work.

    ``nbr`` may be the :class:`KnnIndex` of the cloud (:func:`knn_index`): the search then visits only the cells around every
    query (csrc/knn_grid.hip) and returns the same values and indices, bit for bit.  What the kernels do not take falls back
    to the index's cloud."""
    index = nbr if isinstance(nbr, KnnIndex) else None
    if index is not None:
        nbr = index.cloud
    if not _knn_on_kernels(ref, nbr, k, ord, dim, largest):
        return _knn_tensor(ref, nbr, k, ord, dim, largest, sorted)
    n1, n2 = ref.shape[-2], nbr.shape[-2]
    if k > n2:
        raise RuntimeError("selected index k out of range")
    batch = torch.broadcast_shapes(ref.shape[:-2], nbr.shape[:-2])
    if index is None and _GRID_KNN_MIN is not None and n1 >= _GRID_KNN_MIN[0] and n2 >= _GRID_KNN_MIN[1]:
        try:
            index = KnnIndex(nbr)
        except ValueError:                                                            # (non-finite points, the cell cap)
            pass
    if index is not None and index.batch.numel() not in (1, batch.numel()):           # a partly broadcast batch of indices
        index = None
    r, rs = _knn_flat(ref.detach(), batch)
    if index is None:
        n, ns = _knn_flat(nbr.detach(), batch)
        values, indices = _knn_launch(r, rs, n, ns, batch.numel(), k, splits=_splits)
    else:
        order = _grid_order(r.view(-1, n1, 3)) if _order else None
        values, indices = _knn_launch(r, rs, index.flat, index.ns, batch.numel(), k, grid=(index, order))
    values, indices = values.view(batch + (n1, k)), indices.view(batch + (n1, k))
    if torch.is_grad_enabled() and (ref.requires_grad or nbr.requires_grad):
        picked = torch.gather(nbr.expand(batch + (n2, 3)), -2, indices.reshape(batch + (n1 * k, 1)).expand(batch + (n1 * k, 3)))
        values = torch.linalg.norm(ref.unsqueeze(-2) - picked.view(batch + (n1, k, 3)), dim=-1)
    return torch.return_types.topk((values, indices))


# ---- point-cloud filters (csrc/cloud_filter.hip)
_CF_MAXD = 8
_CF_PARTIAL_SIG = [ctypes.c_void_p] * 4 + [ctypes.c_int64] * 2 + [ctypes.c_double] + [ctypes.c_int] * 2 + [ctypes.c_void_p]
_CF_FINISH_SIG = [ctypes.c_void_p] * 6 + [ctypes.c_int64] * 2 + [ctypes.c_int] * 4 + [ctypes.c_void_p]
_CF_KEYS_SIG = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int] + [ctypes.c_double] * 3 + [ctypes.c_void_p] * 4
_CF_HEADS_SIG = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
_CF_REDUCE_SIG = [ctypes.c_void_p] * 10 + [ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]


def _filter_on_kernels(points, width, ord=2, kk=0):
    """the kernels take HIP clouds (fp32 / fp64) of row width 3..8 whose first three columns are the coordinates, the Euclidean
    norm and lists of at most 16; everything else is the tensor formulation's"""
    return (_C._test_backend is None and points.is_cuda and points.dtype in _C._SUFFIX and ord == 2 and width == 3
            and 3 <= points.shape[-1] <= _CF_MAXD and 0 < points.shape[-2] < 2 ** 31 and kk <= _KNN_MAXK
            and 0 < points.shape[:-2].numel() <= 65535)


def _radius2(radius, dtype):
    """r^2 = radius * radius rounded once in the cloud's dtype, or None where the kernels' d^2 <= r^2 would not be the
    reference's d <= radius (a negative, infinite or NaN radius, an r^2 that overflows)"""
    r = torch.tensor(float(radius), dtype=dtype)
    r2 = (r * r).item()
    return r2 if radius >= 0 and r2 != float("inf") and r2 == r2 else None


def _filter_index(xyz, r2, kk, grid):
    """the :class:`KnnIndex` through which the neighbour filters search ``xyz [B, N, 3]``, or None for the brute-force route.
    ``grid``: a KnnIndex of these columns (used), True (built; None where the index refuses the cloud), False, or None:
    built from ``_GRID_FILTER_MIN_N[kk > 0]`` points, and used unless the cell box of the radius covers so much of the grid that the
    estimated pairs per query -- the occupancy times the box's cells -- exceed ``_GRID_FILTER_BOX_SHARE * N``.  No host read
    beyond the index's own."""
    B, N = xyz.shape[:2]
    if isinstance(grid, KnnIndex):
        if (grid.batch.numel(), grid.n2, grid.cloud.dtype, grid.cloud.device) != (B, N, xyz.dtype, xyz.device):
            raise ValueError("pypose_amd: _grid is not an index of this cloud's coordinate columns")
        return grid
    if grid is False or (grid is None and (_GRID_FILTER_MIN_N is None or N < _GRID_FILTER_MIN_N[kk > 0])):
        return None
    try:
        index = KnnIndex(xyz)
    except ValueError:                                                                # (non-finite points, the cell cap)
        return None
    if grid is None and r2 >= 0:
        h, g = index.header_host[:, 3], index.header_host[:, 4:7]
        reach = 2 * torch.ceil(math.sqrt(r2) / h) + 2                                 # cells per axis, a cell of slack
        pairs = N / g.prod(dim=1) * torch.minimum(g, reach.unsqueeze(1)).prod(dim=1)
        if pairs.max().item() > _GRID_FILTER_BOX_SHARE * N:
            return None
    return index


def _nbr_counts_grid(index, r2, stop, B, N):
    """int32 ``[B, 1, N]``: the points within ``sqrt(r2)`` of every point of the index's cloud (itself included), in original
    order (csrc/nbr_grid.hip); a count is exact unless it exceeds ``stop``"""
    dev, sfx = index.planes.device, _C._SUFFIX[index.planes.dtype]
    pcount = torch.empty((B, 1, N), dtype=torch.int32, device=dev)
    _C.check(_C.library().symbol("pplie_nbr_grid" + sfx, _NBR_GRID_SIG)(
        index.planes.data_ptr(), index.oidx.data_ptr(), index.starts.data_ptr(), index.header.data_ptr(), index.cbase.data_ptr(),
        pcount.data_ptr(), r2, stop, B, N, _C.stream_ptr(dev)), "pplie_nbr_grid" + sfx)
    return pcount


def _nbr_launch(points, r2, kk, nbr, splits=None, grid=None):
    """self-neighbourhood pass and finish on ``points [B, N, D]``: the keep mask ``[B, N]`` (count - 1 >= nbr) and, for
    ``kk > 0``, the mean ``[B, N, D]`` over every point's kk nearest (itself among them).  ``grid`` as :func:`_filter_index`
    takes it: counts and lists then come from the grid kernels (one split each) and the finish is the same."""
    B, N, D = points.shape
    dev, dt = points.device, points.dtype
    cloud = points.contiguous()
    xyz = cloud if D == 3 else points[..., :3].contiguous()
    lib, sfx = _C.library(), _C._SUFFIX[dt]
    ptr = lambda t: None if t is None else t.data_ptr()                               # noqa: E731
    nbr = max(-2 ** 31, min(math.ceil(nbr), 2 ** 31 - 1))                             # (counts are integers below 2^31)
    with _C._on_device(dev):
        st = _C.stream_ptr(dev)
        index = _filter_index(xyz, r2, kk, grid)
        S = splits if splits is not None else -(-512 // (B * -(-N // _KNN_BLOCK)))    # about two workgroups per CU
        S = 1 if index is not None else max(1, min(S, -(-N // _KNN_TILE)))
        pd2 = torch.empty((B, S, N, kk), dtype=dt, device=dev) if kk else None
        pidx = torch.empty((B, S, N, kk), dtype=torch.int32, device=dev) if kk else None
        mask = torch.empty((B, N), dtype=torch.uint8, device=dev)
        mean = torch.empty((B, N, D), dtype=dt, device=dev) if kk else None
        if index is None:
            pcount = torch.empty((B, S, N), dtype=torch.int32, device=dev)
            _C.check(lib.symbol("pplie_nbr_partial" + sfx, _CF_PARTIAL_SIG)(xyz.data_ptr(), pcount.data_ptr(), ptr(pd2), ptr(pidx), B, N,
                                                                            r2, kk, S, st), "pplie_nbr_partial" + sfx)
        else:
            # (without a radius nothing reads the mask: no count launch, as r2 = -1 counts nothing on the brute-force route)
            pcount = _nbr_counts_grid(index, r2, nbr, B, N) if r2 >= 0 else torch.zeros((B, 1, N), dtype=torch.int32, device=dev)
            if kk:                                   # the cloud against its own index, in the index's own order
                _C.check(lib.symbol("pplie_knn_grid" + sfx, _GRID_QUERY_SIG)(
                    index.flat.data_ptr(), None, index.perm.data_ptr(), index.planes.data_ptr(), index.oidx.data_ptr(),
                    index.starts.data_ptr(), index.header.data_ptr(), index.cbase.data_ptr(), pd2.data_ptr(), pidx.data_ptr(),
                    B, N, B * N, kk, index.ns, index.ns, 1 if index.ns else 0, st), "pplie_knn_grid" + sfx)
        _C.check(lib.symbol("pplie_nbr_finish" + sfx, _CF_FINISH_SIG)(pcount.data_ptr(), ptr(pd2), ptr(pidx), ptr(cloud if kk else None),
                                                                      mask.data_ptr(), ptr(mean), B, N, D, kk, S, nbr, st),
                 "pplie_nbr_finish" + sfx)
    return mask.bool(), mean


def _nbr_count_tensor(xyz, radius, ord):
    """``#{j : |x_i - x_j| <= radius}`` (the point itself included) the reference's way, in chunks of rows"""
    n = xyz.shape[-2]
    chunk = max(1, _KNN_CHUNK // max(1, n * xyz.shape[-1]))
    return torch.cat([(torch.linalg.norm(xyz[i:i + chunk].unsqueeze(-2) - xyz.unsqueeze(-3), dim=-1, ord=ord) <= radius).sum(-1)
                      for i in range(0, n, chunk)]) if n else xyz.new_zeros((0,), dtype=torch.int64)


def nbr_filter(points, nbr, radius, pdim=None, ord=2, return_mask=False, _splits=None, _grid=None):
    """Drop the points of ``points (N, D)`` that have fewer than ``nbr`` neighbours within ``radius`` (``ord``-norm over the first
    ``pdim`` columns, default all of them): the kept rows in input order and, with ``return_mask``, the mask ``(N,)`` (reference
    geometry.py:436-493).  Point i is kept when ``#{j : d(i, j) <= radius} - 1 >= nbr``, the count including i itself.

    HIP clouds (fp32 / fp64) with ``pdim == 3``, ``ord == 2`` and ``3 <= D <= 8`` run in csrc/cloud_filter.hip: the cloud is
    streamed against itself through LDS and the ``[N, N]`` distance matrix is never formed.  The kernel compares
    ``d^2 <= r^2`` with ``r^2 = radius * radius`` rounded once in the cloud's dtype, which can differ from the reference's
    ``sqrt(...) <= radius`` only for pairs within a few ulp of the radius.  Everything else takes the tensor formulation.

    ``_grid``: search through a uniform grid over the coordinate columns (csrc/nbr_grid.hip: only the cells within the radius are
    visited; the same mask) -- True builds a :class:`KnnIndex` of them, a KnnIndex of them is used, False never, None decides by
    size (``_GRID_FILTER_MIN_N``).  A cloud the index refuses (non-finite points) takes the brute-force route."""
    assert len(points.shape) == 2, "The point cloud dimension has to be 2."
    pdim = points.size(-1) if pdim is None else pdim
    assert points.size(-1) >= pdim, "The last dim of points should not less than pdim."
    r2 = _radius2(radius, points.dtype) if _filter_on_kernels(points, pdim, ord) else None
    if r2 is not None:
        mask = _nbr_launch(points.detach().unsqueeze(0), r2, 0, nbr, _splits, _grid)[0][0]
    else:
        mask = _nbr_count_tensor(points[..., :pdim].detach(), radius, ord) - 1 >= nbr
    return (points[mask], mask) if return_mask else points[mask]


def random_filter(points, num):
    """``num`` points of ``points (..., N, D)`` drawn without replacement, the same draw for every batch element:
    ``(..., num, D)`` (reference geometry.py:496-527)."""
    assert points.size(-1) >= 1, "The last dim of the points should not less than 1."
    assert num <= points.size(-2), "Number of points to sample must not larger than the number of input points."
    indices = torch.randperm(points.size(-2))[:num]
    return points[..., indices, :]


def _voxel_tensor(points, voxel, random):
    """the reference's result from torch.unique over the int64 cell triples (any device, width and dtype)"""
    vdim = len(voxel)
    xyz = points[..., :vdim]
    cells = ((xyz - xyz.min(dim=-2).values) / torch.tensor(voxel, dtype=torch.float32, device=points.device)).to(torch.int64)
    uniq, inverse, counts = torch.unique(cells, dim=-2, return_inverse=True, return_counts=True)
    if random:
        order = torch.argsort(inverse, stable=True)
        pick = (torch.rand(counts.shape[0], device=points.device) * counts).long().clamp(max=counts - 1)
        return points[order[pick + torch.cumsum(counts, dim=0) - counts]]
    sums = points.new_zeros((uniq.shape[0], points.shape[-1])).index_add_(0, inverse, points)
    return sums / counts.to(points.dtype).view(-1, 1)


def _voxel_launch(cloud, voxel):
    """keys, sort and segmented mean on ``cloud [N, D]``: (means ``[M, D]``, the sort's permutation ``[N]``, start ``[M]``,
    count ``[M]`` of every cell's run in the sorted order), cells in ascending (i0, i1, i2); None when a cell index does not
    fit 21 bits.  One host read: M together with the overflow flag."""
    N, D = cloud.shape
    dev, dt = cloud.device, cloud.dtype
    lib, sfx = _C.library(), _C._SUFFIX[dt]
    nwg = -(-N // 256)
    keys = torch.empty(N, dtype=torch.int64, device=dev)
    part = torch.empty((256, 3), dtype=dt, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    heads = torch.empty(nwg, dtype=torch.int32, device=dev)
    v = [float(torch.tensor(s, dtype=torch.float32)) for s in voxel]                  # rounded to float32, as the reference's
    if not all(0 < s < float("inf") for s in v):
        return None
    with _C._on_device(dev):
        st = _C.stream_ptr(dev)
        _C.check(lib.symbol("pplie_voxel_keys" + sfx, _CF_KEYS_SIG)(cloud.data_ptr(), N, D, v[0], v[1], v[2], part.data_ptr(),
                                                                    keys.data_ptr(), flag.data_ptr(), st), "pplie_voxel_keys" + sfx)
        keys, perm = torch.sort(keys, stable=True)
        _C.check(lib.symbol("pplie_voxel_heads", _CF_HEADS_SIG)(keys.data_ptr(), N, heads.data_ptr(), st), "pplie_voxel_heads")
        total = torch.cumsum(heads, dim=0)
        base = total - heads
        M, bad = torch.stack([total[-1], flag[0].to(torch.int64)]).tolist()
        if bad:
            return None
        out = torch.empty((M, D), dtype=dt, device=dev)
        start = torch.empty(M, dtype=torch.int32, device=dev)
        count = torch.empty(M, dtype=torch.int32, device=dev)
        lead = torch.empty((nwg, 16), dtype=torch.float64, device=dev)
        tail = torch.empty((nwg, 16), dtype=torch.float64, device=dev)
        info = torch.empty((nwg, 4), dtype=torch.int32, device=dev)
        _C.check(lib.symbol("pplie_voxel_reduce" + sfx, _CF_REDUCE_SIG)(keys.data_ptr(), perm.data_ptr(), cloud.data_ptr(), base.data_ptr(),
                                                                        lead.data_ptr(), tail.data_ptr(), info.data_ptr(), out.data_ptr(),
                                                                        start.data_ptr(), count.data_ptr(), N, D, st),
                 "pplie_voxel_reduce" + sfx)
    return out, perm, start, count


def voxel_filter(points, voxel, random=False):
    """One point per occupied voxel of ``points (N, D)``: the mean of all D columns of the voxel's points, or with ``random`` one
    of them; ``(M, D)`` (reference geometry.py:530-602).  ``voxel`` lists the cell sizes of the first ``len(voxel)`` columns.  The
    cell of a point is ``trunc((p - min) / v)`` with ``min`` the column minima of the cloud and ``v`` the sizes rounded to float32
    (the reference builds ``torch.tensor(voxel)``); rows come in ascending lexicographic order of the cell indices, the order of
    ``torch.unique(dim=-2)``.

    HIP clouds (fp32 / fp64) with three positive voxel sizes and ``3 <= D <= 8`` run in csrc/cloud_filter.hip: the cell indices
    (bit-identical to the tensor formulation's) are packed into one int64 key of 3 x 21 bits, sorted, and the means come from a
    segmented scan in fp64 with a fixed order -- no floating-point atomics, two calls give the same bits.  With ``random`` the
    member is drawn with ``torch.rand`` over the run lengths; it is not the reference's draw.  A cloud with more than 2^21
    cells along a column, and everything else, takes the tensor formulation; so does a cloud that records a gradient."""
    assert len(points.shape) == 2, "The point cloud dimension has to be 2."
    D, vdim = points.size(-1), len(voxel)
    assert D >= vdim, "The last dimension of the pointcloud should exceed the dimenson of the voxel space."
    assert all(item != 0 for item in voxel), "Voxel size should be nonzero."
    if _filter_on_kernels(points, vdim) and all(item > 0 for item in voxel) and not (torch.is_grad_enabled() and points.requires_grad):
        res = _voxel_launch(points.detach().contiguous(), voxel)
        if res is not None:
            out, perm, start, count = res
            if not random:
                return out
            pick = (torch.rand(count.shape[0], device=points.device) * count).long().clamp(max=count - 1)
            return points[perm[start + pick]]
    return _voxel_tensor(points, voxel, random)


def _knn_mean_tensor(points, xyz, kk, ord):
    """mean over every point's kk nearest (itself among them), searched in and gathered from the whole cloud"""
    idx = _knn_tensor(xyz, xyz, kk, ord, -1, False, True).indices
    n, D = points.shape[-2:]
    picked = torch.gather(points, -2, idx.reshape(idx.shape[:-2] + (n * kk, 1)).expand(idx.shape[:-2] + (n * kk, D)))
    return picked.view(points.shape[:-1] + (kk, D)).mean(dim=-2)


def knn_filter(points, k, pdim=None, radius=None, ord=2, _splits=None, _grid=None):
    """Smooth ``points (..., N, D)``: every point becomes the mean, over all D columns, of itself and its ``k`` nearest
    neighbours (``ord``-norm over the first ``pdim`` columns); with ``radius`` (then ``points`` is ``(N, D)``) only the points
    with at least ``k`` neighbours within ``radius`` are kept, in input order (reference geometry.py:605-664).

    The k + 1 nearest are searched in the whole input cloud, the point itself among them, and are gathered from it by original
    index; the mean is written for the survivors only.  (The reference gathers from the already compacted cloud with indices of
    the uncompacted one, which agrees with this where the survivors form a prefix of the cloud, as in its example.)  Equal
    distances go to the smaller index.

    HIP clouds (fp32 / fp64) with ``pdim == 3``, ``ord == 2``, ``3 <= D <= 8`` and ``k + 1 <= 16`` run in csrc/cloud_filter.hip:
    one streaming pass over the pairs keeps the count under the radius (``d^2 <= r^2``, ``r^2 = radius * radius`` rounded once in
    the cloud's dtype) next to the best k + 1, and the means are accumulated in fp64.  Everything else, and a cloud that records
    a gradient, takes the tensor formulation.

    ``_grid`` as in :func:`nbr_filter`: the count comes from csrc/nbr_grid.hip and the lists from the cloud's own index
    (csrc/knn_grid.hip), bit for bit the brute-force pass's, so the result is the same."""
    if radius is not None:
        assert len(points.shape) == 2, "The points dimension has to be 2 given radius."
    else:
        assert len(points.shape) >= 2, "The points dimension cannot be less than 2."
    pdim = points.size(-1) if pdim is None else pdim
    assert points.size(-1) >= pdim, "The last dim of points should not less than pdim."
    n, D = points.shape[-2:]
    on_kernels = _filter_on_kernels(points, pdim, ord, k + 1) and k >= 0 and not (torch.is_grad_enabled() and points.requires_grad)
    r2 = -1.0 if radius is None else _radius2(radius, points.dtype) if on_kernels else None
    if k + 1 > n and n > 0:
        raise RuntimeError("selected index k out of range")
    if on_kernels and r2 is not None:
        mask, mean = _nbr_launch(points.detach().reshape(-1, n, D), r2, k + 1, k, _splits, _grid)
        return mean.view(points.shape) if radius is None else mean[0][mask[0]]
    xyz = points[..., :pdim]
    mean = _knn_mean_tensor(points, xyz, k + 1, ord)
    return mean if radius is None else mean[_nbr_count_tensor(xyz.detach(), radius, ord) - 1 >= k]


def _centred(points):
    centre = points.mean(dim=-2, keepdim=True)
    return points - centre, centre


def svdtf(source, target):
    """Rigid transform (SE3) that best maps the point cloud ``source [..., N, 3]`` onto ``target [..., N, 3]`` in the
    least-squares sense, by the SVD of the cross-covariance (Kabsch; reference geometry.py:315-358).  A reflection
    (det = -1) is flipped to the nearest rotation the way the reference does (R -> -R)."""
    from ..lietensor.convert import mat2SE3
    assert source.size(-2) == target.size(-2), {"The number of points N has to be the same for both point clouds."}
    src, c_src = _centred(source)
    tgt, c_tgt = _centred(target)
    U, _, Vh = torch.linalg.svd(torch.einsum('...Na, ...Nb -> ...ab', tgt, src))
    R = U @ Vh
    mirrored = (R.det() + 1).abs() < 1e-6
    R[mirrored] = -R[mirrored]
    t = c_tgt.mT - R @ c_src.mT
    return mat2SE3(torch.cat((R, t), dim=-1), check=False)


def svdstf(source, target, with_scale=True):
    """Similarity transform (Sim3: scale, rotation, translation) that best maps ``source [..., N, 3]`` onto
    ``target [..., N, 3]`` (Umeyama 1991; reference geometry.py:361-433); ``with_scale=False`` fixes the scale to 1."""
    from ..lietensor.convert import mat2Sim3
    assert source.size(-2) == target.size(-2), {"The number of points N has to be the same for both point clouds."}
    assert source.size(-1) == 3, {"The source point dim should be 3"}
    assert target.size(-1) == 3, {"The target point dim should be 3"}
    N, m = source.shape[-2:]
    src, c_src = _centred(source)
    tgt, c_tgt = _centred(target)
    U, D, Vh = torch.linalg.svd(tgt.transpose(-2, -1) @ src / N)
    flip = torch.eye(m, dtype=U.dtype, device=U.device).expand_as(U).clone()      # diag(1, 1, det(U Vh)): proper rotation
    flip[..., -1, -1] = torch.sign(torch.det(U @ Vh))
    if with_scale:
        spread = (src.norm(dim=-1) ** 2).mean(dim=-1, keepdim=True)
        scale = torch.sum(torch.diagonal(flip, dim1=-1, dim2=-2) * D, keepdim=True, dim=-1) / spread
    else:
        scale = torch.ones_like(D[..., 0:1])
    scale = scale.unsqueeze(-1)
    R = U @ flip @ Vh
    t = c_tgt.transpose(-2, -1) - scale * R @ c_src.transpose(-2, -1)
    return mat2Sim3(torch.cat((scale * R, t), dim=-1), check=True)

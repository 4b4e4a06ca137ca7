"""The edges of the Snavely / BAL kernels (csrc/bal.hip) on the MI355X: every output inside guard zones, every operand off
the 16-byte alignment (the VEC=false element-by-element instantiations), exactly full and ragged last tiles, a NULL uv in the
lin kernel, n == 0, the return codes, and the isolation of rows of one LDS tile from a neighbour with a zero depth or nan.

The launcher here resolves the entry points as function/geometry.py _bal_call does but takes the outputs from the caller."""
import contextlib
import ctypes

import pytest
import torch

import pypose_amd as pp
from pypose_amd import _C
from pypose_amd.function import geometry as geo
from tests.bal_util import FWD_TILE, TILE, wide_inputs
from tests.oracle_backend import oracle_row_op

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENTINEL = {torch.float32: (torch.int32, 0x4B4C4D4E), torch.float64: (torch.int64, 0x4B4C4D4E4F505152)}      # finite in both
OFFSETS = {torch.float32: (1, 2, 3), torch.float64: (1,)}          # elements: a base that is not a multiple of 16 bytes
N_TILE = [1, 3, 4, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 3]
N_FWD = [FWD_TILE - 1, FWD_TILE, FWD_TILE + 1]
KERNELS = {  # name: (signature, input widths, output widths, sizes)
    "se3_bal_fwd": (geo._BAL_FWD_SIG, (3, 7, 3, 2), (2,), N_FWD),
    "se3_bal_lin": (geo._BAL_LIN_SIG, (3, 7, 3, 2), (2, 24), N_TILE),
    "bal_vjp": (geo._BAL_VJP_SIG, (24, 2), (3, 7, 3), N_TILE),
}
DTYPES = [torch.float32, torch.float64]
CASES = [(name, dtype, has_uv) for name in KERNELS for dtype in DTYPES for has_uv in (True, False)
         if has_uv or name != "bal_vjp"]                          # vjp takes no uv


def bits(t):
    return t.view(SENTINEL[t.dtype][0])


def carve(n, w, dtype, offset=0, values=None):
    """an [n, w] view at element 64 + offset of a flat buffer filled with the sentinel, 64 sentinels at least on each side;
    torch's allocations start on 512 bytes, so the view's base is 16-byte aligned exactly when offset * itemsize is"""
    ity, pattern = SENTINEL[dtype]
    buf = torch.full((GUARD + offset + n * w + GUARD,), pattern, dtype=ity, device=DEV).view(dtype)
    assert buf.data_ptr() % 16 == 0
    view = buf[GUARD + offset:GUARD + offset + n * w].view(n, w)
    assert (view.data_ptr() % 16 != 0) == (offset * buf.element_size() % 16 != 0)
    if values is not None:
        view.copy_(values)
    return buf, view


def guards_intact(buf, view):
    ity, pattern = SENTINEL[buf.dtype]
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    b = bits(buf)
    return lo >= GUARD and len(b) - lo - view.numel() >= GUARD and bool((b[:lo] == pattern).all()) \
        and bool((b[lo + view.numel():] == pattern).all())


def launch(name, ins, outs, n):
    """``pplie_<name>_{f32,f64}`` resolved as geometry._bal_call does; inputs and outputs are the caller's (``None``: NULL)"""
    first = next(t for t in ins if t is not None)
    fn = _C.library().symbol("pplie_" + name + _C._SUFFIX[first.dtype], KERNELS[name][0])
    with _C._on_device(first.device):
        return fn(*[None if t is None else t.data_ptr() for t in (*ins, *outs)], n, _C.stream_ptr(first.device))


@pytest.fixture(scope="module")
def data():
    """dtype -> (K, X, p, uv, g) of 600 wide rows on the device; J comes from the ordinary lin call"""
    out = {}
    for dtype in DTYPES:
        rows = [t.to(DEV) for t in wide_inputs(600, dtype, seed=7)]
        g = torch.randn(600, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(8)).to(dtype).to(DEV)
        out[dtype] = (*rows, g)
    return out


def operands(name, data, dtype, n, has_uv):
    """the inputs of one launch and the result of the ordinary call (fresh, aligned allocations)"""
    K, X, p, uv, g = [t[:n].contiguous() for t in data[dtype]]
    uv = uv if has_uv else None
    if name == "se3_bal_fwd":
        return [K, X, p, uv], [geo._bal_fwd(K, X, p, uv)]
    if name == "se3_bal_lin":
        return [K, X, p, uv], list(geo._bal_lin(K, X, p, uv))
    J = geo._bal_lin(K, X, p, uv)[1]
    return [J, g], list(geo._bal_vjp(J, g))


def run_carved(name, ins, want, n, offsets):
    """launch with every operand carved at its offset, outputs between guards; the payload equals ``want`` bit for bit"""
    widths = KERNELS[name][1] + KERNELS[name][2]
    dtype = want[0].dtype
    k = len(ins)
    cin = [None if t is None else carve(n, w, dtype, o, t)[1] for t, w, o in zip(ins, widths[:k], offsets[:k])]
    cout = [carve(n, w, dtype, o) for w, o in zip(widths[k:], offsets[k:])]
    for t, o in zip(cin + [v for _, v in cout], offsets):
        assert t is None or (t.data_ptr() % 16 != 0) == (o != 0)
    assert launch(name, cin, [v for _, v in cout], n) == 0
    for i, ((buf, view), ref) in enumerate(zip(cout, want)):
        assert guards_intact(buf, view), (name, n, offsets, "output", i)
        assert torch.equal(bits(view), bits(ref)), (name, n, offsets, "output", i)
    for t, src in zip(cin, ins):
        assert t is None or torch.equal(bits(t), bits(src))                      # inputs are read only


@pytest.mark.parametrize("name,dtype,has_uv", CASES)
def test_outputs_stay_inside_guard_zones(data, name, dtype, has_uv):
    """aligned bases (the dwordx4 slab path; the ragged last tile stores element by element): nothing outside the payload
    changes and the payload is the ordinary call's"""
    nops = len(KERNELS[name][1]) + len(KERNELS[name][2])
    for n in KERNELS[name][3]:
        ins, want = operands(name, data, dtype, n, has_uv)
        run_carved(name, ins, want, n, [0] * nops)


@pytest.mark.parametrize("name,dtype,has_uv", CASES)
def test_unaligned_operands_give_the_same_bits(data, name, dtype, has_uv):
    """one operand at a time, then all of them, off the 16-byte alignment: the element-by-element kernels (VEC=false) run the
    same per-row arithmetic (the file is built without packed fp32), so the results are those of the aligned launch bit for
    bit -- and stay inside their guard zones"""
    nops = len(KERNELS[name][1]) + len(KERNELS[name][2])
    for n in KERNELS[name][3]:
        ins, want = operands(name, data, dtype, n, has_uv)
        present = [i for i in range(nops) if i >= len(ins) or ins[i] is not None]
        for off in OFFSETS[dtype]:
            for i in present:
                run_carved(name, ins, want, n, [off if j == i else 0 for j in range(nops)])
            run_carved(name, ins, want, n, [off] * nops)
        if len(OFFSETS[dtype]) > 1:
            run_carved(name, ins, want, n, [OFFSETS[dtype][j % 3] for j in range(nops)])       # every operand its own offset


@pytest.mark.parametrize("dtype", DTYPES)
def test_lin_with_null_uv(data, dtype):
    for n in N_TILE + N_FWD:
        K, X, p, uv, _ = [t[:n].contiguous() for t in data[dtype]]
        r0, J0 = geo._bal_lin(K, X, p, None)
        assert torch.equal(bits(r0), bits(geo._bal_fwd(K, X, p, None)))
        assert torch.equal(bits(J0), bits(geo._bal_lin(K, X, p, uv)[1]))
        assert torch.equal(bits(geo._bal_lin(K, X, p, uv)[0]), bits(geo._bal_fwd(K, X, p, uv)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_observations(dtype):
    K = torch.zeros(0, 3, dtype=dtype, device=DEV, requires_grad=True)
    C = pp.Parameter(pp.SE3(torch.zeros(0, 7, dtype=dtype, device=DEV)))
    P = torch.zeros(0, 3, dtype=dtype, device=DEV, requires_grad=True)
    uv = torch.zeros(0, 2, dtype=dtype, device=DEV, requires_grad=True)
    r = pp.bal_reprojerr(P, uv, K, C)
    assert r.shape == (0, 2) and r.dtype == dtype and r.is_cuda
    grads = torch.autograd.grad(r.sum(), [K, C, P, uv])
    assert [tuple(g.shape) for g in grads] == [(0, 3), (0, 7), (0, 3), (0, 2)]
    with torch.no_grad():
        assert pp.bal_reprojerr(P, uv, K, C).shape == (0, 2) and pp.bal_point2pixel(P, K, C).shape == (0, 2)
        assert pp.bal_reprojerr(P, uv, K, C, reduction='norm').shape == (0,)
    assert [tuple(t.shape) for t in geo._bal_lin(K.detach(), C.detach().tensor(), P.detach())] == [(0, 2), (0, 24)]
    assert [tuple(t.shape) for t in geo._bal_vjp(torch.zeros(0, 24, dtype=dtype, device=DEV), uv.detach())] == [(0, 3), (0, 7), (0, 3)]


@pytest.mark.parametrize("suffix", ["_f32", "_f64"])
def test_bad_arguments_return_codes(suffix):
    null, stream = ctypes.c_void_p(0), _C.stream_ptr(torch.device(DEV))
    buf = torch.zeros(5 * 24, dtype=torch.float64, device=DEV)                  # large enough for any operand of 5 rows
    ptr = ctypes.c_void_p(buf.data_ptr())
    for name, (sig, iw, ow, _) in KERNELS.items():
        fn = _C.library().symbol("pplie_" + name + suffix, sig)
        nptr = len(iw) + len(ow)
        assert fn(*[null] * nptr, ctypes.c_int64(-1), stream) == -1             # PPLIE_EBADARG
        assert fn(*[ptr] * nptr, ctypes.c_int64(-1), stream) == -1
        assert fn(*[null] * nptr, ctypes.c_int64(0), stream) == 0               # PPLIE_OK: nothing to do, nothing dereferenced
        assert fn(*[null] * nptr, ctypes.c_int64(5), stream) == -1
        optional = {3} if name != "bal_vjp" else set()                         # uv may be NULL
        for i in set(range(nptr)) - optional:
            args = [null if j == i or j in optional else ptr for j in range(nptr)]
            assert fn(*args, ctypes.c_int64(5), stream) == -1, (name, i)
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0


@contextlib.contextmanager
def composed_on_device():
    """a stand-in back end (the numpy oracle, results moved to the inputs' device): bal_reprojerr takes the composed route"""
    _C.set_backend_for_testing(lambda name, ins, ow, prm=None: tuple(o.to(ins[0].device) for o in oracle_row_op(name, ins, ow, prm)))
    try:
        yield
    finally:
        _C.set_backend_for_testing(None)


@pytest.mark.parametrize("dtype", DTYPES)
def test_poison_rows_do_not_leak_into_their_tile(data, dtype):
    """Rows 0, TILE-1, TILE and n-1 of a benign batch become a zero depth (k1 > 0 > k2 and the reverse), a zero camera-frame
    point and a nan K.  Every other row of r, J, gK, gX, gp keeps its bits: an LDS pitch or index error that finite
    neighbours hide would smear the non-finite values.  The poison rows are non-finite in the kernel and in the composed
    model; the patterns need not be the same and are not (bal_math.h: Horner form against inf - inf = nan; on the MI355X the
    zero-depth rows are +-inf in fp32 and nan in fp64, whose reciprocal is the approximate one; the composed model has nan)."""
    n = 2 * TILE + 3
    K, X, p, uv, g = [t[:n].clone() for t in data[dtype]]
    clean_r, clean_J = geo._bal_lin(K, X, p, uv)
    clean_g = geo._bal_vjp(clean_J, g)
    rows = [0, TILE - 1, TILE, n - 1]
    eye = torch.tensor([0, 0, 0, 0, 0, 0, 1], dtype=dtype, device=DEV)
    X[rows[0]], X[rows[1]], X[rows[2]] = eye, eye, eye
    p[rows[0]] = p[rows[1]] = torch.tensor([0.3, -0.2, 0.0], dtype=dtype, device=DEV)
    p[rows[2]] = 0
    K[rows[0]] = torch.tensor([500, 0.1, -0.01], dtype=dtype, device=DEV)
    K[rows[1]] = torch.tensor([500, -0.1, 0.01], dtype=dtype, device=DEV)
    K[rows[3]] = float("nan")
    r, J = geo._bal_lin(K, X, p, uv)
    grads = geo._bal_vjp(J, g)
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[rows] = False
    for got, want in zip((r, J, *grads, geo._bal_fwd(K, X, p, uv)), (clean_r, clean_J, *clean_g, clean_r)):
        assert torch.equal(bits(got)[keep], bits(want)[keep])
    assert not torch.isfinite(r[rows]).any(), r[rows]
    print(dtype, "kernel", r[rows].tolist())
    assert (~torch.isfinite(J[rows])).any(-1).all()
    assert float(grads[1][:, 6].abs().max()) == 0
    with composed_on_device():
        rc = pp.bal_reprojerr(p, uv, K, pp.SE3(X))
    assert not torch.isfinite(rc[rows]).any(), rc[rows]
    print(dtype, "composed", rc[rows].tolist())

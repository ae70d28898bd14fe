"""ttr_mode_diff and ttr_laplace_core through the C ABI on a real MI355X, against the fp64 pass of the host mirror on the CPU
applied to the same (rounded) input: 5e-6 (fp32) / 1e-12 (fp64) of the largest reference entry -- every pass is one subtraction
and one scaling, so orders up to 5 stay well inside.  Shapes: odd sizes, C = 1 (the last core), R = 1 (the first core, a Tucker
factor), I = 1 and 2, C a multiple of the 16-byte vector and not, and more than one block."""
import ctypes

import pytest
import torch

from tntorch_amd import _hip as h
from tntorch_amd import _hostops

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
SHAPES = [(3, 5, 7), (1, 5, 3), (3, 5, 1), (1, 2, 1), (1, 1, 4), (2, 3, 17), (17, 65, 3), (1, 64, 64), (64, 64, 64)]
INV = 1.75   # 1 / step


def _i64(values):
    return (ctypes.c_int64 * len(values))(*[int(v) for v in values])


def _bound(dt):
    return 5e-6 if dt == torch.float32 else 1e-12


def _input(shape, dt, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g, dtype=torch.float64).to(dt)


def _close(out, ref, dt, what):
    err = float((out.cpu().double() - ref).abs().max())
    scale = float(ref.abs().max())
    print(what, dt, "error", err, "largest entry", scale)
    assert err <= _bound(dt) * scale, (what, err, scale)


@pytest.fixture(scope="module")
def fused():
    return h.mode_diff_max_order()


def test_fused_limit(fused):
    assert fused == 4


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_mode_diff(shape, periodic, dt, fused):
    X = _input(shape, dt)
    Xd = X.cuda()
    for order in (1, 2, 3, fused + 1):   # the last one: a fused launch of `fused` passes chained with one more
        ref = _hostops.mode_diff(X.double(), order, periodic, INV)
        out = h.mode_diff(Xd, order, periodic, INV)
        assert out.is_cuda and out.dtype == dt and tuple(out.shape) == shape
        _close(out, ref, dt, "mode_diff {} order {} periodic {}".format(shape, order, periodic))
    assert torch.equal(Xd.cpu(), X)   # the input is left alone


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape, pad", [((3, 5, 7), (2, 3, 5)), ((2, 6, 8), (1, 2, 4)), ((1, 4, 1), (0, 1, 3))])
def test_mode_diff_strided_output_leaves_the_rest_alone(shape, pad, dt):
    """Y is a block of a larger buffer filled with a sentinel: every element outside the block is still the sentinel."""
    R, I, C = shape
    X = _input(shape, dt, seed=1)
    big = torch.full((R + 2 * pad[0], I + 2 * pad[1], C + 2 * pad[2]), -77.0, dtype=dt).cuda()
    view = big[pad[0]:pad[0] + R, pad[1]:pad[1] + I, pad[2]:pad[2] + C]
    for order in (2, 5):
        big.fill_(-77.0)
        got = h.mode_diff(X.cuda(), order, False, INV, out=view)
        assert got.data_ptr() == view.data_ptr()
        _close(view, _hostops.mode_diff(X.double(), order, False, INV), dt, "strided {} order {}".format(shape, order))
        mask = torch.ones(big.shape, dtype=torch.bool)
        mask[pad[0]:pad[0] + R, pad[1]:pad[1] + I, pad[2]:pad[2] + C] = False
        assert bool((big.cpu()[mask] == -77.0).all())


@pytest.mark.parametrize("dt", DTYPES)
def test_mode_diff_refusals_leave_the_output_untouched(dt):
    L = h.lib()
    code = h.dtype_code(dt)
    X = _input((3, 5, 7), dt).cuda()
    Y = torch.full((3, 5, 7), -77.0, dtype=dt).cuda()
    xs, ys = _i64(X.stride()), _i64(Y.stride())

    def call(R=3, I=5, C=7, order=1, x=X, xstr=xs, y=Y, ystr=ys):
        return L.ttr_mode_diff(code, R, I, C, order, 0, INV, x.data_ptr(), xstr, y.data_ptr(), ystr, None)

    Xt = _input((7, 5, 3), dt).cuda().permute(2, 1, 0)   # [3, 5, 7] but not contiguous
    assert call(x=Xt, xstr=_i64(Xt.stride())) == h.E_UNSUPPORTED
    assert call(xstr=_i64((35, 8, 1))) == h.E_UNSUPPORTED
    assert call(y=X) == h.E_INVALID                                   # X == Y
    assert call(order=0) == h.E_INVALID
    assert call(order=-1) == h.E_INVALID
    assert call(I=0) == h.E_INVALID
    assert call(order=h.mode_diff_max_order() + 1) == h.E_UNSUPPORTED     # above the fused limit: the caller chains
    assert call(ystr=_i64((35, 6, 1))) == h.E_UNSUPPORTED                 # si < C
    assert call(ystr=_i64((30, 7, 1))) == h.E_UNSUPPORTED                 # sr < I si
    assert call(ystr=_i64((35, 7, 2))) == h.E_UNSUPPORTED                 # last stride not 1
    assert L.ttr_mode_diff(7, 3, 5, 7, 1, 0, INV, X.data_ptr(), xs, Y.data_ptr(), ys, None) == h.E_INVALID
    assert L.ttr_mode_diff(code, 3, 5, 7, 1, 0, INV, None, xs, Y.data_ptr(), ys, None) == h.E_INVALID
    torch.cuda.synchronize()
    assert bool((Y.cpu() == -77.0).all())
    with pytest.raises(NotImplementedError):
        h.mode_diff(Xt, 1, False, INV)
    with pytest.raises(ValueError):
        h.mode_diff(X, 0, False, INV)
    assert call() == 0   # and the same arguments without a fault go through
    _close(Y, _hostops.mode_diff(X.cpu().double(), 1, False, INV), dt, "after the refusals")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_laplace_core(shape, periodic, dt):
    R, I, C = shape
    X = _input(shape, dt, seed=2)
    Xd = X.cuda()
    D = _hostops.mode_diff(X.double(), 2, periodic, INV)
    for pos in (0, 1, 2):
        out = h.laplace_core(Xd, pos, periodic, INV)
        want = {0: (R, I, 2 * C), 1: (2 * R, I, 2 * C), 2: (2 * R, I, C)}[pos]
        assert out.is_cuda and out.dtype == dt and tuple(out.shape) == want and out.is_contiguous()
        o = out.cpu()
        if pos == 2:
            a_blocks, d_block = [o[R:]], o[:R]
        else:
            a_blocks, d_block = [o[:R, :, :C]], o[:R, :, C:]
            if pos == 1:
                a_blocks.append(o[R:, :, C:])
                zero = o[R:, :, :C]
                assert not zero.any() and not torch.signbit(zero).any()   # exactly (+) zero
        for a in a_blocks:
            assert torch.equal(a, X)   # bit-identical copies of the input
        _close(d_block, D, dt, "laplace_core {} pos {} periodic {}".format(shape, pos, periodic))
        ref = _hostops.laplace_core(X.double(), pos, periodic, INV)
        _close(out, ref, dt, "laplace_core against the mirror")


def test_laplace_core_refusals():
    L = h.lib()
    X = _input((3, 5, 7), torch.float32).cuda()
    out = torch.full((6, 5, 14), -77.0).cuda()
    xs = _i64(X.stride())
    assert L.ttr_laplace_core(h.F32, 3, 5, 7, 3, 0, INV, X.data_ptr(), xs, out.data_ptr(), None) == h.E_INVALID     # pos
    assert L.ttr_laplace_core(h.F32, 3, 0, 7, 1, 0, INV, X.data_ptr(), xs, out.data_ptr(), None) == h.E_INVALID     # I = 0
    assert L.ttr_laplace_core(h.F32, 3, 5, 7, 1, 0, INV, X.data_ptr(), xs, X.data_ptr(), None) == h.E_INVALID       # X == out
    assert L.ttr_laplace_core(h.F32, 3, 5, 7, 1, 0, INV, X.data_ptr(), _i64((35, 1, 5)), out.data_ptr(), None) == h.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out.cpu() == -77.0).all())

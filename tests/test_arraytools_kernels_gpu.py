"""ttr_mode_scan and ttr_mode_reduce through the C ABI on a real MI355X, in both dtypes.  The truth is the operation in fp64 on the
CPU applied to the input as rounded to the dtype; the bounds are entry-wise and derived (arraytools_cases.kernel_bound), with A
the same operation on the absolute values:

    fp64   scan  I 2^-52 A          reduce  (I + 2) 2^-52 A        (any summation order, with a factor 2 to spare)
    fp32   + 2^-23 |truth|, the one rounding at the store

Shapes (R, I, C): both edge cores, C below / at / above a wave, vector-aligned and not, I that splits unevenly over the waves of a
workgroup and their row groups, more than one workgroup."""
import ctypes
import re

import pytest
import torch

import arraytools_cases as ac
from tntorch_amd import _hip as h

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
SENTINEL = -77.0


def _i64(values):
    return (ctypes.c_int64 * len(values))(*[int(v) for v in values])


def _within(out, truth, bound, what):
    err = (out.cpu().double() - truth).abs()
    worst = float((err - bound).max())
    print(what, "largest error", float(err.max()), "largest bound", float(bound.max()), "largest excess", worst)
    assert bool((err <= bound).all()), (what, float(err.max()), worst)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", ac.KERNEL_SHAPES)
def test_mode_scan(shape, dt):
    X, _ = ac.kernel_input(shape, dt)
    Xd = X.cuda()
    truth, A = ac.scan_truth(X)
    out = h.mode_scan(Xd)
    assert out.is_cuda and out.dtype == dt and tuple(out.shape) == shape and out.is_contiguous()
    _within(out, truth, ac.kernel_bound("scan", shape[1], dt, truth, A), "mode_scan {} {}".format(shape, dt))
    again = h.mode_scan(Xd)
    assert torch.equal(out, again)          # bit-identical from call to call
    assert torch.equal(Xd.cpu(), X)         # the input is left alone


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", ac.KERNEL_SHAPES)
def test_mode_reduce(shape, dt):
    R, I, C = shape
    X, w = ac.kernel_input(shape, dt, seed=1)
    Xd, wd = X.cuda(), w.cuda()
    for weights, scale in ((wd, 1.0), (wd, -0.375), (None, 1.0 / I)):
        truth, A = ac.reduce_truth(X, None if weights is None else w, scale)
        out = h.mode_reduce(Xd, weights, scale)
        assert out.is_cuda and out.dtype == dt and tuple(out.shape) == (R, C) and out.is_contiguous()
        _within(out, truth, ac.kernel_bound("reduce", I, dt, truth, A),
                "mode_reduce {} {} w {} scale {}".format(shape, dt, weights is not None, scale))
        assert torch.equal(out, h.mode_reduce(Xd, weights, scale))   # bit-identical from call to call
    assert torch.equal(h.mode_reduce(Xd, None, 0.5), h.mode_reduce(Xd, torch.ones(I, dtype=dt).cuda(), 0.5))   # NULL is all ones
    assert torch.equal(Xd.cpu(), X) and torch.equal(wd.cpu(), w)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape, pad", [((3, 5, 7), (2, 3, 5)), ((2, 6, 8), (1, 2, 4)), ((1, 4, 1), (0, 1, 3)), ((2, 70, 4), (1, 1, 4)),
                                        ((1, 600, 8), (1, 2, 3))])
def test_strided_output_leaves_the_rest_alone(shape, pad, dt):
    """Y is a block of a larger buffer filled with a sentinel: every element outside the block is still the sentinel.  (The
    blocks are aligned to 16 bytes or not; the last one goes through the kernels that split I over the waves of a workgroup.)"""
    R, I, C = shape
    X, w = ac.kernel_input(shape, dt, seed=2)
    big = torch.full((R + 2 * pad[0], I + 2 * pad[1], C + 2 * pad[2]), SENTINEL, dtype=dt).cuda()
    view = big[pad[0]:pad[0] + R, pad[1]:pad[1] + I, pad[2]:pad[2] + C]
    got = h.mode_scan(X.cuda(), out=view)
    assert got.data_ptr() == view.data_ptr()
    truth, A = ac.scan_truth(X)
    _within(view, truth, ac.kernel_bound("scan", I, dt, truth, A), "strided scan {}".format(shape))
    assert torch.equal(view.contiguous(), h.mode_scan(X.cuda()))    # the same bits wherever the result goes
    mask = torch.ones(big.shape, dtype=torch.bool)
    mask[pad[0]:pad[0] + R, pad[1]:pad[1] + I, pad[2]:pad[2] + C] = False
    assert bool((big.cpu()[mask] == SENTINEL).all())

    big2 = torch.full((R + 2 * pad[0], C + 2 * pad[2]), SENTINEL, dtype=dt).cuda()
    view2 = big2[pad[0]:pad[0] + R, pad[2]:pad[2] + C]
    h.mode_reduce(X.cuda(), w.cuda(), 1.5, out=view2)
    truth, A = ac.reduce_truth(X, w, 1.5)
    _within(view2, truth, ac.kernel_bound("reduce", I, dt, truth, A), "strided reduce {}".format(shape))
    assert torch.equal(view2.contiguous(), h.mode_reduce(X.cuda(), w.cuda(), 1.5))
    mask2 = torch.ones(big2.shape, dtype=torch.bool)
    mask2[pad[0]:pad[0] + R, pad[2]:pad[2] + C] = False
    assert bool((big2.cpu()[mask2] == SENTINEL).all())


@pytest.mark.parametrize("dt", DTYPES)
def test_refusals_leave_the_output_untouched(dt):
    L = h.lib()
    code = h.dtype_code(dt)
    X, w = ac.kernel_input((3, 5, 7), dt)
    X, w = X.cuda(), w.cuda()
    Y = torch.full((3, 5, 7), SENTINEL, dtype=dt).cuda()
    Z = torch.full((3, 7), SENTINEL, dtype=dt).cuda()
    xs, ys, zs = _i64(X.stride()), _i64(Y.stride()), _i64(Z.stride())
    Xt = ac.kernel_input((7, 5, 3), dt)[0].cuda().permute(2, 1, 0)   # [3, 5, 7] but not contiguous

    def scan(R=3, I=5, C=7, x=X, xstr=xs, y=Y, ystr=ys, dtype=code):
        return L.ttr_mode_scan(dtype, R, I, C, x.data_ptr() if x is not None else None, xstr, y.data_ptr(), ystr, None)

    def reduce(R=3, I=5, C=7, x=X, xstr=xs, y=Z, ystr=zs, dtype=code):
        return L.ttr_mode_reduce(dtype, R, I, C, x.data_ptr() if x is not None else None, xstr, w.data_ptr(), 1.0, y.data_ptr(), ystr, None)

    for f in (scan, reduce):
        assert f(x=Xt, xstr=_i64(Xt.stride())) == h.E_UNSUPPORTED        # a permuted X
        assert f(xstr=_i64((35, 8, 1))) == h.E_UNSUPPORTED
        assert f(y=X) == h.E_INVALID                                      # X == Y
        assert f(I=0) == h.E_INVALID
        assert f(R=0) == h.E_INVALID
        assert f(C=-1) == h.E_INVALID
        assert f(dtype=7) == h.E_INVALID
        assert f(x=None) == h.E_INVALID
    assert scan(ystr=_i64((35, 6, 1))) == h.E_UNSUPPORTED                 # si < C
    assert scan(ystr=_i64((30, 7, 1))) == h.E_UNSUPPORTED                 # sr < I si
    assert scan(ystr=_i64((35, 7, 2))) == h.E_UNSUPPORTED                 # last stride not 1
    assert reduce(ystr=_i64((6, 1))) == h.E_UNSUPPORTED                   # sr < C
    assert reduce(ystr=_i64((7, 2))) == h.E_UNSUPPORTED                   # last stride not 1
    torch.cuda.synchronize()
    assert bool((Y.cpu() == SENTINEL).all()) and bool((Z.cpu() == SENTINEL).all())
    with pytest.raises(NotImplementedError):
        h.mode_scan(Xt)
    with pytest.raises(NotImplementedError):
        h.mode_reduce(Xt)
    with pytest.raises(ValueError):
        h.mode_reduce(X, w[:4])
    assert scan() == 0 and reduce() == 0   # and the same arguments without a fault go through
    truth, A = ac.scan_truth(X)
    _within(Y, truth, ac.kernel_bound("scan", 5, dt, truth, A), "scan after the refusals")
    truth, A = ac.reduce_truth(X, w, 1.0)
    _within(Z, truth, ac.kernel_bound("reduce", 5, dt, truth, A), "reduce after the refusals")


def test_symbols_are_declared_and_exported():
    with open(h._HEADER) as f:
        header = f.read()
    for name in ("ttr_mode_scan", "ttr_mode_reduce"):
        assert re.search(r"\bint\s+{}\s*\(".format(name), header), name
        assert name in h.EXPORTED_SYMBOLS and hasattr(h.lib(), name)

"""ttr_core_convolve through the C ABI on a real MI355X, fp32 and fp64, against the fp64 host mirror on the same (rounded) inputs.

Per entry  |out - ref| <= (min(I, J) + 2) u absconv,  absconv the mirror applied to |a| and |c|, u = 2^-24 / 2^-53: a sum of n
products accumulates at most n rounding errors, plus the one at the store (derived, not measured).

The shapes (convolve_cases.KERNEL_SHAPES) straddle the kernel's limits: the column tile of 64 (63, 64, 65, 66 and 68 columns; 35
columns: no multiple of 4), the k tiles of 16 (single-element stores), 32 (16-byte stores in fp64) and 64 (16-byte stores in
fp32) with K one below, at and one above each, the staged limit of ttr_core_convolve_max_taps() = 32 terms of the sum over the
shorter mode (31, 32, 33 and 65 terms, either argument the shorter one), mode sizes of 1, a first and a last core, and one case
of 64 rows x 2 k tiles.  Every shape runs the full, same and valid windows and the interior window (lo, K) = (2, 3)."""
import functools

import pytest
import torch

import convolve_cases as cc
from tntorch_amd import _hip as h

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
SENTINEL = -77.0
GUARD = 64   # elements: 256 / 512 bytes, the output stays 16-byte aligned


@functools.lru_cache(maxsize=None)
def _case(sa, sc, dt):
    """Inputs (CPU, rounded to dt) and, per window, the fp64 reference and bound: computed once per shape and dtype."""
    a, c = cc.kernel_inputs(sa, sc, dt)
    refs = []
    for lo, K in cc.kernel_windows(sa[1], sc[1]):
        ref = cc.mirror64(a, c, lo, K)
        bound = cc.kernel_bound(sa[1], sc[1], dt, cc.mirror64(a.abs(), c.abs(), lo, K))
        refs.append((lo, K, ref, bound))
    return a, c, refs


def _raw(L, dt, sa, sc, lo, K, a, c, out_ptr):
    return L.ttr_core_convolve(h.dtype_code(dt), sa[0], sa[1], sa[2], sc[0], sc[1], sc[2], lo, K, a.data_ptr(), c.data_ptr(), out_ptr, None)


def _check(out, ref, bound, what):
    diff = (out.cpu().double().reshape(ref.shape) - ref).abs()
    worst = float((diff / bound.clamp_min(1e-300)).max())
    print(what, "largest error / bound", worst)
    assert bool((diff <= bound).all()), (what, worst)


def test_staged_limit():
    assert h.core_convolve_max_taps() == 32


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("sa, sc", cc.KERNEL_SHAPES)
def test_core_convolve(sa, sc, dt):
    """The output lies in a sentinel-filled buffer with guards before and after it: exactly R1 S1 K R2 S2 elements are written,
    the guards and the inputs stay as they were, and a second call gives the same bits."""
    L = h.lib()
    a, c, refs = _case(sa, sc, dt)
    ad, cd = a.cuda(), c.cuda()
    item = ad.element_size()
    for lo, K, ref, bound in refs:
        n = sa[0] * sc[0] * K * sa[2] * sc[2]
        buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=dt, device="cuda")
        assert _raw(L, dt, sa, sc, lo, K, ad, cd, buf.data_ptr() + GUARD * item) == 0, L.ttr_last_error()
        first = buf.cpu()
        assert bool((first[:GUARD] == SENTINEL).all()) and bool((first[GUARD + n:] == SENTINEL).all())
        _check(first[GUARD:GUARD + n], ref, bound, "{} x {} window ({}, {}) {}".format(sa, sc, lo, K, dt))
        buf.fill_(SENTINEL)
        assert _raw(L, dt, sa, sc, lo, K, ad, cd, buf.data_ptr() + GUARD * item) == 0
        assert torch.equal(buf.cpu(), first)   # bit-identical, guards included
        out = h.core_convolve(ad, cd, lo, K)    # the wrapper: same bits in a fresh tensor
        assert out.is_cuda and out.dtype == dt and tuple(out.shape) == (sa[0] * sc[0], K, sa[2] * sc[2]) and out.is_contiguous()
        assert torch.equal(out.cpu().reshape(-1), first[GUARD:GUARD + n])
    assert torch.equal(ad.cpu(), a) and torch.equal(cd.cpu(), c)


@pytest.mark.parametrize("dt", DTYPES)
def test_output_that_is_not_16_byte_aligned(dt):
    """64 columns, but the output starts one element past a 16-byte boundary: single-element stores, nothing outside."""
    L = h.lib()
    sa, sc = (1, 17, 8), (1, 16, 8)
    a, c, refs = _case(sa, sc, dt)
    ad, cd = a.cuda(), c.cuda()
    lo, K, ref, bound = refs[0]
    n = K * 64
    buf = torch.full((GUARD + 1 + n + GUARD,), SENTINEL, dtype=dt, device="cuda")
    assert _raw(L, dt, sa, sc, lo, K, ad, cd, buf.data_ptr() + (GUARD + 1) * ad.element_size()) == 0
    got = buf.cpu()
    assert bool((got[:GUARD + 1] == SENTINEL).all()) and bool((got[GUARD + 1 + n:] == SENTINEL).all())
    _check(got[GUARD + 1:GUARD + 1 + n], ref, bound, "unaligned output {}".format(dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_refusals_leave_the_output_untouched(dt):
    L = h.lib()
    sa, sc = (3, 5, 7), (2, 4, 3)
    a, c, refs = _case(sa, sc, dt)
    ad, cd = a.cuda(), c.cuda()
    out = torch.full((6 * 8 * 21,), SENTINEL, dtype=dt, device="cuda")
    code = h.dtype_code(dt)

    def call(dtype=code, R1=3, I=5, R2=7, S1=2, J=4, S2=3, lo=0, K=8, pa=ad.data_ptr(), pc=cd.data_ptr(), po=out.data_ptr()):
        return L.ttr_core_convolve(dtype, R1, I, R2, S1, J, S2, lo, K, pa, pc, po, None)

    assert call(dtype=7) == h.E_INVALID
    for name in ("R1", "I", "R2", "S1", "J", "S2", "K"):
        assert call(**{name: 0}) == h.E_INVALID, name
    assert call(lo=-1) == h.E_INVALID
    assert call(lo=1, K=8) == h.E_INVALID          # lo + K > I + J - 1
    assert call(lo=0, K=9) == h.E_INVALID
    assert call(lo=8, K=1) == h.E_INVALID
    assert call(pa=None) == h.E_INVALID
    assert call(pc=None) == h.E_INVALID
    assert call(po=None) == h.E_INVALID
    assert call(po=ad.data_ptr()) == h.E_INVALID   # out == a
    assert call(po=cd.data_ptr()) == h.E_INVALID   # out == c
    torch.cuda.synchronize()
    assert bool((out.cpu() == SENTINEL).all())
    assert torch.equal(ad.cpu(), a) and torch.equal(cd.cpu(), c)
    # the wrapper: exceptions for cores that are not contiguous, not 3-d, of two dtypes, and for the library's refusals
    at = a.permute(2, 1, 0).contiguous().cuda().permute(2, 1, 0)   # [3, 5, 7], not contiguous
    with pytest.raises(ValueError):
        h.core_convolve(at, cd, 0, 8)
    with pytest.raises(ValueError):
        h.core_convolve(ad, cd[:, ::2], 0, 6)
    with pytest.raises(ValueError):
        h.core_convolve(ad[0], cd, 0, 8)
    with pytest.raises(ValueError):
        h.core_convolve(ad, cd.to(torch.float64 if dt == torch.float32 else torch.float32), 0, 8)
    with pytest.raises(ValueError):
        h.core_convolve(ad, cd, 1, 8)
    with pytest.raises(ValueError):
        h.core_convolve(ad, cd, 0, 0)
    lo, K, ref, bound = refs[0]
    assert (lo, K) == (0, 8) and call() == 0       # and after the refusals a good call still gives the right answer
    _check(out, ref, bound, "after the refusals")

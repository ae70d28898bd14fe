"""ttr_core_compose through the C ABI on a real MI355X, fp32 and fp64, against the fp64 einsum on the same (rounded) inputs.

Per element  |out - out64| <= 2 (J + 1) u (|A| o |B|)  (algebra_cases: derived, not measured).  The shapes (algebra_cases.SHAPES)
put R1 P R2, S1 Q S2 and R2 S2 one below, at and one above every TTR_COMPOSE_TILE_* extent, J below a quad, across a quad and
across the staged chunk, every axis at 1, runs of 1, 65 and 256 elements, S2 above the column tile, and several tiles on both
sides.  Beyond the values: exactly the output's elements are written (sentinel guards), the same call gives the same bits, and
an element's bits do not depend on where it lies in a tile, on the other extents or on the alignment of the output."""
import functools

import pytest
import torch

import algebra_cases as ac
from tntorch_amd import _hip as h
from tntorch_amd import _hipops

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
SENTINEL = -77.0
GUARD = 64   # elements: 256 / 512 bytes, the output stays 16-byte aligned


@functools.lru_cache(maxsize=None)
def _case(shape, dt):
    """Inputs (CPU, rounded to dt), the fp64 reference and the bound: computed once per shape and dtype."""
    A, B = ac.operands(shape, dt)
    ref, bound = ac.core_truth_and_bound(A, B, dt)
    return A, B, ref, bound


def _raw(L, dt, A, B, out_ptr):
    R1, P, J, R2 = A.shape
    S1, _, Q, S2 = B.shape
    return L.ttr_core_compose(h.dtype_code(dt), R1, P, J, R2, S1, Q, S2, A.data_ptr(), B.data_ptr(), out_ptr, None)


def _check(out, ref, bound, what):
    diff = (out.cpu().double().reshape(ref.shape) - ref).abs()
    worst = float((diff / bound.clamp_min(1e-300)).max())
    print(what, "largest error / bound", worst)
    assert bool((diff <= bound).all()), (what, worst)


def test_tile_extents():
    assert (h.COMPOSE_TILE_M, h.COMPOSE_TILE_N, h.COMPOSE_TILE_K) == (64, 64, 32)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", ac.SHAPES)
def test_core_compose(shape, dt):
    """The output lies in a sentinel-filled buffer with guards before and after it: exactly its elements are written, the guards
    and the inputs stay as they were, a second call gives the same bits, and so does the wrapper in a fresh tensor."""
    L = h.lib()
    A, B, ref, bound = _case(shape, dt)
    Ad, Bd = A.cuda(), B.cuda()
    item, n = Ad.element_size(), ref.numel()
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=dt, device="cuda")
    assert _raw(L, dt, Ad, Bd, buf.data_ptr() + GUARD * item) == 0, L.ttr_last_error()
    first = buf.cpu()
    assert bool((first[:GUARD] == SENTINEL).all()) and bool((first[GUARD + n:] == SENTINEL).all())
    _check(first[GUARD:GUARD + n], ref, bound, "{} {}".format(shape, dt))
    buf.fill_(SENTINEL)
    assert _raw(L, dt, Ad, Bd, buf.data_ptr() + GUARD * item) == 0
    assert torch.equal(buf.cpu(), first)   # bit-identical, guards included
    out = h.core_compose(Ad, Bd)
    assert out.is_cuda and out.dtype == dt and tuple(out.shape) == tuple(ref.shape) and out.is_contiguous()
    assert torch.equal(out.cpu().reshape(-1), first[GUARD:GUARD + n])
    assert torch.equal(Ad.cpu(), A) and torch.equal(Bd.cpu(), B)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", [(16, 2, 2, 16, 16, 2, 16), (3, 5, 70, 9, 4, 3, 7), (5, 1, 4, 13, 3, 1, 5), (2, 1, 6, 3, 1, 2, 80)])
def test_bits_do_not_depend_on_the_position(shape, dt):
    """compose(A[:1], B[:1]) is the block (r = 0, a = 0) of compose(A, B), compose(A[:, :1], B) its slice p = 0, and
    compose(A, B[:, :, :1]) its slice q = 0: other extents, other tiles, other places in them, the same bits."""
    A, B, _, _ = _case(shape, dt)
    Ad, Bd = A.cuda(), B.cuda()
    R1, P, J, R2, S1, Q, S2 = shape
    full = h.core_compose(Ad, Bd).cpu()
    full6 = full.reshape(R1, S1, P, Q, R2, S2)
    one = h.core_compose(Ad[:1].contiguous(), Bd[:1].contiguous()).cpu()
    assert torch.equal(one.reshape(P, Q, R2, S2), full6[0, 0])
    row = h.core_compose(Ad[:, :1].contiguous(), Bd).cpu()
    assert torch.equal(row, full[:, :1])
    col = h.core_compose(Ad, Bd[:, :, :1].contiguous()).cpu()
    assert torch.equal(col, full[:, :, :1])
    last = h.core_compose(Ad[:, :, :, R2 - 1:].contiguous(), Bd[:, :, :, S2 - 1:].contiguous()).cpu()
    assert torch.equal(last.reshape(R1, S1, P, Q), full6[..., R2 - 1, S2 - 1])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", [(16, 2, 2, 16, 16, 2, 16), (3, 1, 5, 2, 4, 6, 8), (3, 5, 70, 9, 4, 3, 7)])
def test_output_one_element_off_a_16_byte_boundary(shape, dt):
    """The scalar stores give the bits of the aligned call's packs, and nothing outside the output is written."""
    L = h.lib()
    A, B, ref, bound = _case(shape, dt)
    Ad, Bd = A.cuda(), B.cuda()
    n = ref.numel()
    aligned = h.core_compose(Ad, Bd)
    assert aligned.data_ptr() % 16 == 0
    buf = torch.full((GUARD + 1 + n + GUARD,), SENTINEL, dtype=dt, device="cuda")
    assert buf.data_ptr() % 16 == 0
    assert _raw(L, dt, Ad, Bd, buf.data_ptr() + (GUARD + 1) * Ad.element_size()) == 0
    got = buf.cpu()
    assert bool((got[:GUARD + 1] == SENTINEL).all()) and bool((got[GUARD + 1 + n:] == SENTINEL).all())
    assert torch.equal(got[GUARD + 1:GUARD + 1 + n], aligned.cpu().reshape(-1))
    _check(got[GUARD + 1:GUARD + 1 + n], ref, bound, "unaligned output {} {}".format(shape, dt))
    # the wrapper with an ``out`` of its own, offset the same way
    out = torch.full((n + 1,), SENTINEL, dtype=dt, device="cuda")
    res = h.core_compose(Ad, Bd, out=out[1:])
    assert res.data_ptr() == out.data_ptr() + Ad.element_size() and torch.equal(res.cpu(), aligned.cpu())
    assert float(out[0]) == SENTINEL


@pytest.mark.parametrize("dt", DTYPES)
def test_views_go_through_hipops(dt):
    """A transposed matrix core and a train core with an inserted axis are not contiguous: the binding refuses them, _hipops
    copies them first and gives the bits of the contiguous call."""
    shape = (4, 6, 5, 5, 3, 5, 2)
    A, B, ref, bound = _case(shape, dt)
    Ad, Bd = A.cuda(), B.cuda()
    want = h.core_compose(Ad, Bd)
    At = Ad.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)   # the same values, strides of a transposed core
    Bt = Bd.permute(3, 1, 2, 0).contiguous().permute(3, 1, 2, 0)
    assert not At.is_contiguous() and not Bt.is_contiguous()
    with pytest.raises(ValueError, match="contiguous"):
        h.core_compose(At, Bd)
    with pytest.raises(ValueError, match="contiguous"):
        h.core_compose(Ad, Bt)
    got = _hipops.core_compose(At, Bt)
    assert torch.equal(got.cpu(), want.cpu())
    _check(got, ref, bound, "views {}".format(dt))
    assert torch.equal(At.cpu(), A) and torch.equal(Bt.cpu(), B)


@pytest.mark.parametrize("dt", DTYPES)
def test_refusals_leave_the_output_untouched(dt):
    L = h.lib()
    shape = (2, 3, 4, 3, 2, 2, 5)
    A, B, ref, bound = _case(shape, dt)
    Ad, Bd = A.cuda(), B.cuda()
    out = torch.full((ref.numel(),), SENTINEL, dtype=dt, device="cuda")
    code = h.dtype_code(dt)

    def call(dtype=code, R1=2, P=3, J=4, R2=3, S1=2, Q=2, S2=5, pa=Ad.data_ptr(), pb=Bd.data_ptr(), po=out.data_ptr()):
        return L.ttr_core_compose(dtype, R1, P, J, R2, S1, Q, S2, pa, pb, po, None)

    assert call(dtype=7) == h.E_INVALID
    for name in ("R1", "P", "J", "R2", "S1", "Q", "S2"):
        assert call(**{name: 0}) == h.E_INVALID, name
    assert call(pa=None) == h.E_INVALID and call(pb=None) == h.E_INVALID and call(po=None) == h.E_INVALID
    assert call(po=Ad.data_ptr()) == h.E_INVALID and call(po=Bd.data_ptr()) == h.E_INVALID
    assert call(J=1 << 31) == h.E_UNSUPPORTED
    assert call(R1=1 << 16, S1=1 << 16) == h.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out.cpu() == SENTINEL).all())
    with pytest.raises(ValueError):
        h.core_compose(Ad[0], Bd)
    with pytest.raises(ValueError):
        h.core_compose(Ad, Bd.to(torch.float64 if dt == torch.float32 else torch.float32))
    with pytest.raises(ValueError, match="the same J"):
        h.core_compose(Ad, Bd[:, :3].contiguous())
    with pytest.raises(ValueError, match="out must be"):
        h.core_compose(Ad, Bd, out=out[:-1])
    assert call() == 0                     # and after the refusals a good call still gives the right answer
    _check(out, ref, bound, "after the refusals")
    assert torch.equal(Ad.cpu(), A) and torch.equal(Bd.cpu(), B)

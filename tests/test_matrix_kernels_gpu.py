"""ttr_ttm_step and ttr_cpm_step through the C ABI on a real MI355X, in both dtypes.  The truth is the step in fp64 on the CPU from
the operands as rounded to the dtype; the bound is entry-wise and derived (matrix_cases: 2 (K + 1) u (|X| . |G|), K = I R for the
TT step and I for the CP step).  Y always lies between two guard regions filled with a sentinel that are compared bit for bit
afterwards; every launch stays in bounds.

Shapes (matrix_cases.TTM_SHAPES): D below / at / above a row tile and a workgroup tile, K < 4, quads of k that straddle two
input indices (R = 3, 5, 33), K and N across their tiles, N < 16 and N = 16; one shape per instance (R a power of two or not)
where every tile loop runs at least three times."""
import ctypes
import re

import pytest
import torch

import matrix_cases as mc
from tntorch_amd import _hip as h

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
SENTINEL = -77.0
GUARD = 300   # elements in front of and behind Y


def _i64(values):
    return (ctypes.c_int64 * len(values))(*[int(v) for v in values])


def _guarded(numel, dt, offset=0):
    """(buffer, view of `numel` elements starting GUARD + offset elements in): the buffer is all sentinel."""
    buf = torch.full((numel + 2 * GUARD + offset,), SENTINEL, dtype=dt).cuda()
    return buf, buf[GUARD + offset:GUARD + offset + numel]


def _guards_intact(buf, numel, offset=0):
    host = buf.cpu()
    return bool((host[:GUARD + offset] == SENTINEL).all()) and bool((host[GUARD + offset + numel:] == SENTINEL).all())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", mc.TTM_SHAPES + [mc.TTM_BIG, mc.TTM_BIG_P2])
def test_ttm_step(shape, dt):
    I, D, R, O, S = shape
    X, G = mc.ttm_operands(shape, dt)
    Xd, Gd = X.cuda(), G.cuda()
    truth, bound = mc.ttm_truth_and_bound(X, G, dt)
    buf, Y = _guarded(D * O * S, dt)
    out = h.ttm_step(Xd, Gd, out=Y)
    assert out.data_ptr() == Y.data_ptr()
    mc.assert_within(Y.view(D, O, S), truth, bound, "ttm_step {} {}".format(shape, dt))
    assert _guards_intact(buf, D * O * S)
    fresh = h.ttm_step(Xd, Gd)
    assert fresh.is_cuda and fresh.dtype == dt and tuple(fresh.shape) == (D, O, S) and fresh.is_contiguous()
    assert torch.equal(fresh.reshape(-1), Y)          # the same bits from call to call, wherever the result goes
    assert torch.equal(Xd.cpu(), X) and torch.equal(Gd.cpu(), G)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("which", ["X", "G", "Y"])
def test_ttm_step_without_16_byte_alignment(which, dt):
    """R and N are multiples of 16 bytes of elements, but one operand starts one element past a 16-byte boundary: that tile is
    loaded element by element, with the same arithmetic -- the same bits as the aligned call -- and the guards around Y stay."""
    shape = (3, 70, 8, 2, 4)
    I, D, R, O, S = shape
    X, G = mc.ttm_operands(shape, dt)
    aligned = h.ttm_step(X.cuda(), G.cuda())

    def shifted(t):
        store = torch.empty(t.numel() + 1, dtype=dt).cuda()
        view = store[1:].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 != 0
        return view

    Xd = shifted(X) if which == "X" else X.cuda()
    Gd = shifted(G) if which == "G" else G.cuda()
    off = 1 if which == "Y" else 0
    buf, Y = _guarded(D * O * S, dt, offset=off)
    h.ttm_step(Xd, Gd, out=Y)
    assert torch.equal(Y, aligned.reshape(-1))
    assert _guards_intact(buf, D * O * S, offset=off)
    truth, bound = mc.ttm_truth_and_bound(X, G, dt)
    mc.assert_within(aligned, truth, bound, "ttm_step {} {}".format(shape, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_ttm_step_layout_with_exact_data(dt):
    """Small integers: every product and sum is exact, so the result must EQUAL the truth -- a swapped row / column map of the
    accumulators or a wrong (i, r) -> row of G would show here whatever the tolerance.  G is far from symmetric."""
    I, D, R, O, S = 3, 70, 5, 7, 3
    X = ((torch.arange(I * D * R) * 7) % 11 - 5).to(dt).reshape(I, D, R)
    G = ((torch.arange(R * I * O * S) * 5) % 13 - 6).to(dt).reshape(R, I, O, S)
    truth = torch.einsum("idr,rios->dos", X.double(), G.double())
    assert torch.equal(h.ttm_step(X.cuda(), G.cuda()).cpu().double(), truth)


@pytest.mark.parametrize("dt", DTYPES)
def test_ttm_step_output_is_the_next_input(dt):
    """Two chained steps, the second reading the first's output as it lies, against the two-core matrix product."""
    g = torch.Generator().manual_seed(5)
    b, (I0, I1), (O0, O1), r = 19, (6, 5), (3, 4), 7
    G0 = torch.randn((1, I0, O0, r), dtype=torch.float64, generator=g).to(dt)
    G1 = torch.randn((r, I1, O1, 1), dtype=torch.float64, generator=g).to(dt)
    x = torch.randn((b, I0 * I1), dtype=torch.float64, generator=g).to(dt)
    y64, bound = mc.tt_truth_and_bound([G0, G1], x, dt)
    X0 = x.t().contiguous().cuda()
    Y0 = h.ttm_step(X0.view(I0, -1, 1), G0.cuda())
    Y1 = h.ttm_step(Y0.view(I1, -1, r), G1.cuda())
    mc.assert_within(Y1.view(b, -1), y64, bound, "two steps {}".format(dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_ttm_step_refusals_leave_the_output_untouched(dt):
    L = h.lib()
    code = h.dtype_code(dt)
    shape = (3, 5, 4, 2, 6)
    X, G = mc.ttm_operands(shape, dt)
    X, G = X.cuda(), G.cuda()
    Xt = X.permute(1, 0, 2).contiguous().permute(1, 0, 2)          # [I, D, R] with the strides of [D, I, R]
    Gt = G.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3)    # [R, I, O, S] stored as [I, R, O, S]
    buf, Y = _guarded(5 * 2 * 6, dt)
    before = buf.clone()

    def call(dtype=code, I=3, D=5, R=4, O=2, S=6, x=X, xstr=None, g=G, gstr=None, y=Y):
        xs = xstr if xstr is not None else (_i64(x.stride()) if x is not None else None)
        gs = gstr if gstr is not None else (_i64(g.stride()) if g is not None else None)
        return L.ttr_ttm_step(dtype, I, D, R, O, S, x.data_ptr() if x is not None else None, xs, g.data_ptr() if g is not None else None,
                              gs, y.data_ptr() if y is not None else None, None)

    assert call(x=Xt) == h.E_UNSUPPORTED                 # a permuted X
    assert call(g=Gt) == h.E_UNSUPPORTED                 # a permuted G
    assert call(xstr=_i64((20, 4, 2))) == h.E_UNSUPPORTED
    assert call(gstr=_i64((36, 12, 7, 1))) == h.E_UNSUPPORTED
    assert call(y=X) == h.E_INVALID                      # X == Y
    assert call(dtype=7) == h.E_INVALID
    for name in ("I", "D", "R", "O", "S"):
        assert call(**{name: 0}) == h.E_INVALID, name
    assert call(D=-3) == h.E_INVALID
    assert call(x=None) == h.E_INVALID and call(g=None) == h.E_INVALID and call(y=None) == h.E_INVALID
    assert call(D=2 ** 31) == h.E_UNSUPPORTED            # refused from the sizes alone, before anything is read
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    assert call(I=1, D=1, xstr=_i64((999, 999, 1)), gstr=_i64((12, 999, 6, 1))) == 0   # the stride of an extent-1 axis is free
    torch.cuda.synchronize()
    with pytest.raises(NotImplementedError):
        h.ttm_step(Xt, G)
    with pytest.raises(NotImplementedError):
        h.ttm_step(X, Gt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("x_has_rank", [0, 1])
@pytest.mark.parametrize("shape", mc.CPM_SHAPES)
def test_cpm_step(shape, x_has_rank, dt):
    I, D, O, R = shape
    X, C = mc.cpm_operands(shape, dt, x_has_rank)
    Xd, Cd = X.cuda(), C.cuda()
    truth, bound = mc.cpm_truth_and_bound(X, C, dt)
    buf, Y = _guarded(D * O * R, dt)
    h.cpm_step(Xd, Cd, out=Y)
    mc.assert_within(Y.view(D, O, R), truth, bound, "cpm_step {} rank axis {} {}".format(shape, x_has_rank, dt))
    assert _guards_intact(buf, D * O * R)
    fresh = h.cpm_step(Xd, Cd)
    assert fresh.is_cuda and fresh.dtype == dt and tuple(fresh.shape) == (D, O, R) and fresh.is_contiguous()
    assert torch.equal(fresh.reshape(-1), Y)
    assert torch.equal(Xd.cpu(), X) and torch.equal(Cd.cpu(), C)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("which", ["X", "C", "Y"])
def test_cpm_step_without_16_byte_alignment(which, dt):
    """One operand starts one element past a 16-byte boundary: the scalar instance runs, with the same arithmetic -- the same
    bits as the aligned call -- and the guards around Y stay."""
    shape = (3, 65, 2, 8)
    I, D, O, R = shape
    X, C = mc.cpm_operands(shape, dt, 1)
    aligned = h.cpm_step(X.cuda(), C.cuda())

    def shifted(t):
        store = torch.empty(t.numel() + 1, dtype=dt).cuda()
        view = store[1:].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 != 0
        return view

    Xd = shifted(X) if which == "X" else X.cuda()
    Cd = shifted(C) if which == "C" else C.cuda()
    off = 1 if which == "Y" else 0
    buf, Y = _guarded(D * O * R, dt, offset=off)
    assert (Y.data_ptr() % 16 != 0) == (which == "Y")
    h.cpm_step(Xd, Cd, out=Y)
    assert torch.equal(Y, aligned.reshape(-1))
    assert _guards_intact(buf, D * O * R, offset=off)


@pytest.mark.parametrize("dt", DTYPES)
def test_cpm_step_refusals_leave_the_output_untouched(dt):
    L = h.lib()
    code = h.dtype_code(dt)
    X, C = mc.cpm_operands((3, 5, 2, 4), dt, 1)
    X, C = X.cuda(), C.cuda()
    buf, Y = _guarded(5 * 2 * 4, dt)
    before = buf.clone()

    def call(dtype=code, I=3, D=5, O=2, R=4, xr=1, x=X, c=C, y=Y):
        return L.ttr_cpm_step(dtype, I, D, O, R, xr, x.data_ptr() if x is not None else None, c.data_ptr() if c is not None else None,
                              y.data_ptr() if y is not None else None, None)

    assert call(y=X) == h.E_INVALID and call(y=C) == h.E_INVALID
    assert call(dtype=7) == h.E_INVALID
    for name in ("I", "D", "O", "R"):
        assert call(**{name: 0}) == h.E_INVALID, name
    assert call(xr=2) == h.E_INVALID
    assert call(x=None) == h.E_INVALID and call(c=None) == h.E_INVALID and call(y=None) == h.E_INVALID
    assert call(D=2 ** 58) == h.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    with pytest.raises(ValueError):
        h.cpm_step(X.permute(1, 0, 2).contiguous().permute(1, 0, 2), C)   # the binding refuses what the entry cannot express


def test_entries_are_declared_and_exported():
    with open(h._HEADER) as f:
        header = f.read()
    for name in ("ttr_ttm_step", "ttr_cpm_step"):
        assert re.search(r"\bint\s+{}\s*\(".format(name), header), name
        assert name in h.EXPORTED_SYMBOLS and hasattr(h.lib(), name)

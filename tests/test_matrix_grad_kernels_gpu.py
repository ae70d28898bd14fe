"""ttr_ttm_grad_input and ttr_ttm_grad_core through the C ABI on a real MI355X, in both dtypes.  The truth is the einsum in fp64 on
the CPU from the operands as rounded to the dtype; the bounds are entry-wise and derived (matrix_grad_cases:
2 (O S + 1) u (|dY| . |G|) and 2 (D + 1) u (|X|^T . |dY|), the latter for any summation order, so it covers the slab sum).  Every
output lies between two guard regions filled with a sentinel that are compared bit for bit afterwards, and every call runs twice:
the bits must be equal.

Shapes: the (I, R) x (O, S) x D grid of matrix_cases.TTM_SHAPES and its two large shapes for grad_input (N = I R and K = O S below /
at / across their tiles, runs of r that straddle a tile, R with and without 16-byte packs); for grad_core the same (I, R) x (O, S)
pairs with D around a quad of k, a K tile, a slab (L = ttr_ttm_grad_core_slab_rows), across four slabs and across 11 and 20 (runs of
several slabs in the slab sum, a partial last run, empty runs), and one shape whose slabs are longer than the minimum."""
import ctypes

import pytest
import torch

import matrix_cases as mc
import matrix_grad_cases as gc
from tntorch_amd import _hip as h

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
SENTINEL = -77.0
GUARD = 300   # elements in front of and behind an output
PAIRS = [(I, R, O, S) for I, _, R, O, S in mc.TTM_SHAPES]
# 10L+3 and 19L+1: 11 and 20 slabs, so the eight runs of the slab sum hold 2 resp. 3 slabs, the last live run is partial (1 resp. 2)
# and the runs after it are empty
D_LABELS = ["1", "3", "4", "5", "63", "65", "L-1", "L", "L+1", "3L+5", "10L+3", "19L+1"]


def _guarded(numel, dt, offset=0):
    """(buffer, view of `numel` elements starting GUARD + offset elements in): the buffer is all sentinel."""
    buf = torch.full((numel + 2 * GUARD + offset,), SENTINEL, dtype=dt).cuda()
    return buf, buf[GUARD + offset:GUARD + offset + numel]


def _guards_intact(buf, numel, offset=0):
    host = buf.cpu()
    return bool((host[:GUARD + offset] == SENTINEL).all()) and bool((host[GUARD + offset + numel:] == SENTINEL).all())


def _shifted(t):
    """A device copy of `t` that starts one element past a 16-byte boundary."""
    store = torch.empty(t.numel() + 1, dtype=t.dtype).cuda()
    view = store[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0
    return view


def _ptr(t):
    return t.data_ptr() if t is not None else None


# ------------------------------------------------------------------ ttr_ttm_grad_input
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", mc.TTM_SHAPES + [mc.TTM_BIG, (4, 130, 32, 5, 16)])
def test_grad_input(shape, dt):
    I, D, R, O, S = shape
    _, G, dY = gc.grad_operands(shape, dt)
    Gd, dYd = G.cuda(), dY.cuda()
    truth, bound = gc.grad_input_truth_and_bound(dY, G, dt)
    buf, dX = _guarded(I * D * R, dt)
    out = h.ttm_grad_input(dYd, Gd, out=dX)
    assert out.data_ptr() == dX.data_ptr()
    mc.assert_within(dX.view(I, D, R), truth, bound, "ttm_grad_input {} {}".format(shape, dt))
    assert _guards_intact(buf, I * D * R)
    fresh = h.ttm_grad_input(dYd, Gd)
    assert fresh.is_cuda and fresh.dtype == dt and tuple(fresh.shape) == (I, D, R) and fresh.is_contiguous()
    assert torch.equal(fresh.reshape(-1), dX)            # the same bits from call to call, wherever the result goes
    assert torch.equal(Gd.cpu(), G) and torch.equal(dYd.cpu(), dY)


@pytest.mark.parametrize("dt", DTYPES)
def test_grad_input_layout_with_exact_data(dt):
    """Small integers: every product and sum is exact, so the result must EQUAL the truth -- a swapped row / column map of the
    accumulators, a wrong (i, r) -> row of G or a wrong segment of the store would show whatever the tolerance.  G is far from
    symmetric; N = 15 R-runs of 5 across a tile edge, D across two row tiles."""
    I, D, R, O, S = 15, 70, 5, 7, 3
    dY = gc.small_integers((D, O, S), 7, 11, dt)
    G = gc.small_integers((R, I, O, S), 5, 13, dt)
    truth = torch.einsum("dos,rios->idr", dY.double(), G.double())
    got = h.ttm_grad_input(dY.cuda(), G.cuda())
    assert torch.equal(got.cpu().double(), truth)
    assert torch.equal(h.ttm_grad_input(dY.cuda(), G.cuda()), got)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("which", ["dY", "G", "dX"])
def test_grad_input_without_16_byte_alignment(which, dt):
    """K = O S and R are multiples of 16 bytes of elements, but one operand starts one element past a 16-byte boundary: its
    accesses go element by element, with the same arithmetic -- the same bits as the aligned call -- and the guards stay."""
    shape = (3, 70, 8, 2, 4)
    I, D, R, O, S = shape
    _, G, dY = gc.grad_operands(shape, dt)
    aligned = h.ttm_grad_input(dY.cuda(), G.cuda())
    dYd = _shifted(dY) if which == "dY" else dY.cuda()
    Gd = _shifted(G) if which == "G" else G.cuda()
    off = 1 if which == "dX" else 0
    buf, dX = _guarded(I * D * R, dt, offset=off)
    assert (dX.data_ptr() % 16 != 0) == (which == "dX")
    h.ttm_grad_input(dYd, Gd, out=dX)
    assert torch.equal(dX, aligned.reshape(-1))
    assert _guards_intact(buf, I * D * R, offset=off)
    truth, bound = gc.grad_input_truth_and_bound(dY, G, dt)
    mc.assert_within(aligned, truth, bound, "ttm_grad_input {} {}".format(shape, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_grad_input_refusals_leave_the_output_untouched(dt):
    L = h.lib()
    code = h.dtype_code(dt)
    shape = (3, 5, 4, 2, 6)
    _, G, dY = gc.grad_operands(shape, dt)
    G, dY = G.cuda(), dY.cuda()
    buf, dX = _guarded(3 * 5 * 4, dt)
    before = buf.clone()

    def call(dtype=code, I=3, D=5, R=4, O=2, S=6, dy=dY, g=G, dx=dX):
        return L.ttr_ttm_grad_input(dtype, I, D, R, O, S, _ptr(dy), _ptr(g), _ptr(dx), None)

    assert call(dx=dY) == h.E_INVALID and call(dx=G) == h.E_INVALID      # the output is one of the inputs
    assert call(dtype=7) == h.E_INVALID
    for name in ("I", "D", "R", "O", "S"):
        assert call(**{name: 0}) == h.E_INVALID, name
    assert call(D=-3) == h.E_INVALID
    assert call(dy=None) == h.E_INVALID and call(g=None) == h.E_INVALID and call(dx=None) == h.E_INVALID
    assert call(D=2 ** 31) == h.E_UNSUPPORTED             # refused from the sizes alone, before anything is read
    assert call(I=2 ** 16, R=2 ** 15) == h.E_UNSUPPORTED
    assert call(O=2 ** 16, S=2 ** 15) == h.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    assert call() == 0
    torch.cuda.synchronize()
    assert _guards_intact(buf, 3 * 5 * 4) and not torch.equal(buf, before)
    with pytest.raises(ValueError):
        h.ttm_grad_input(dY.permute(1, 0, 2).contiguous().permute(1, 0, 2), G)   # the binding refuses what the entry cannot express
    with pytest.raises(ValueError):
        h.ttm_grad_input(dY, G.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3))


# ------------------------------------------------------------------ ttr_ttm_grad_core
def _rows(label, L):
    return {"L-1": L - 1, "L": L, "L+1": L + 1, "3L+5": 3 * L + 5, "10L+3": 10 * L + 3, "19L+1": 19 * L + 1}.get(label) or int(label)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("label", D_LABELS)
@pytest.mark.parametrize("pair", PAIRS)
def test_grad_core(pair, label, dt):
    I, R, O, S = pair
    L = h.ttm_grad_core_slab_rows(dt, I, 1, R, O, S)
    assert L >= 4
    D = _rows(label, L)
    shape = (I, D, R, O, S)
    slab = h.ttm_grad_core_slab_rows(dt, *shape)
    nslab = -(-D // slab)
    wsb = h.ttm_grad_core_workspace_bytes(dt, *shape)
    assert slab == L                                      # (at these sizes the rule does not move with D)
    assert nslab == {"L-1": 1, "L": 1, "L+1": 2, "3L+5": 4, "10L+3": 11, "19L+1": 20}.get(label, 1)
    assert wsb == (nslab * I * R * O * S * (4 if dt == torch.float32 else 8) if nslab > 1 else 0)
    X, _, dY = gc.grad_operands(shape, dt)
    Xd, dYd = X.cuda(), dY.cuda()
    truth, bound = gc.grad_core_truth_and_bound(X, dY, dt)
    buf, dG = _guarded(R * I * O * S, dt)
    out = h.ttm_grad_core(Xd, dYd, out=dG.view(R, I, O, S))
    assert out.data_ptr() == dG.data_ptr()
    mc.assert_within(dG.view(R, I, O, S), truth, bound, "ttm_grad_core {} {}".format(shape, dt))
    assert _guards_intact(buf, R * I * O * S)
    fresh = h.ttm_grad_core(Xd, dYd)
    assert fresh.is_cuda and fresh.dtype == dt and tuple(fresh.shape) == (R, I, O, S) and fresh.is_contiguous()
    assert torch.equal(fresh.reshape(-1), dG)             # the same bits from call to call: the slabs are summed in order
    assert torch.equal(Xd.cpu(), X) and torch.equal(dYd.cpu(), dY)
    assert h.ttm_grad_core_slab_rows(dt, *shape) == slab and h.ttm_grad_core_workspace_bytes(dt, *shape) == wsb


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("mult,extra,nslab", [(3, 5, 4), (10, 3, 11), (19, 1, 20)])
def test_grad_core_layout_with_exact_data_across_slabs(mult, extra, nslab, dt):
    """Small integers over 4, 11 and 20 slabs: every product and sum is exact (|sum| <= D * 30 < 2^24), so the result must EQUAL
    the truth, whatever the association of the slab sum -- a run of the sum that drops, repeats or overwrites a slab cannot
    pass (11 slabs: runs of 2, the sixth run has 1, two are empty; 20: runs of 3, the seventh has 2, one is empty).
    M = 15 runs of 5 across a tile edge, N = 21."""
    I, R, O, S = 15, 5, 7, 3
    L = h.ttm_grad_core_slab_rows(dt, I, 1, R, O, S)
    D = mult * L + extra
    assert h.ttm_grad_core_slab_rows(dt, I, D, R, O, S) == L and -(-D // L) == nslab and D * 30 < 2 ** 24
    X = gc.small_integers((I, D, R), 7, 11, dt)
    dY = gc.small_integers((D, O, S), 5, 13, dt)
    truth = torch.einsum("idr,dos->rios", X.double(), dY.double())
    got = h.ttm_grad_core(X.cuda(), dY.cuda())
    assert torch.equal(got.cpu().double(), truth)
    assert torch.equal(h.ttm_grad_core(X.cuda(), dY.cuda()), got)
    one = h.ttm_grad_core(X[:, :L].contiguous().cuda(), dY[:L].cuda())   # one slab: written without the workspace
    assert torch.equal(one.cpu().double(), torch.einsum("idr,dos->rios", X[:, :L].double(), dY[:L].double()))


@pytest.mark.parametrize("dt", DTYPES)
def test_grad_core_slabs_longer_than_the_minimum(dt):
    """Six output tiles and D = 50,000: the rule gives want = 1024 // 6 = 170 slabs, ceil(D / 170) = 295 rows rounded up to 320 > 256,
    so 157 slabs in runs of 20 (the eighth run has 17).  Random data within the bound, small integers exactly (D * 30 < 2^24)."""
    shape = (2, 50000, 33, 5, 26)
    I, D, R, O, S = shape
    slab = h.ttm_grad_core_slab_rows(dt, *shape)
    assert slab == 320 and -(-D // slab) == 157
    assert h.ttm_grad_core_workspace_bytes(dt, *shape) == 157 * I * R * O * S * (4 if dt == torch.float32 else 8)
    X, _, dY = gc.grad_operands(shape, dt)
    truth, bound = gc.grad_core_truth_and_bound(X, dY, dt)
    buf, dG = _guarded(R * I * O * S, dt)
    h.ttm_grad_core(X.cuda(), dY.cuda(), out=dG.view(R, I, O, S))
    mc.assert_within(dG.view(R, I, O, S), truth, bound, "ttm_grad_core {} {}".format(shape, dt))
    assert _guards_intact(buf, R * I * O * S)
    assert torch.equal(h.ttm_grad_core(X.cuda(), dY.cuda()).reshape(-1), dG)
    Xi = gc.small_integers((I, D, R), 7, 11, dt)
    dYi = gc.small_integers((D, O, S), 5, 13, dt)
    exact = torch.einsum("idr,dos->rios", Xi.double(), dYi.double())
    assert torch.equal(h.ttm_grad_core(Xi.cuda(), dYi.cuda()).cpu().double(), exact)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("which", ["X", "dY", "dG"])
@pytest.mark.parametrize("D", [70, 600])
def test_grad_core_without_16_byte_alignment(D, which, dt):
    """R and N = O S are multiples of 16 bytes of elements, but one operand starts one element past a 16-byte boundary: the
    same bits as the aligned call (one slab and three), and the guards stay."""
    shape = (3, D, 8, 2, 4)
    I, _, R, O, S = shape
    X, _, dY = gc.grad_operands(shape, dt)
    aligned = h.ttm_grad_core(X.cuda(), dY.cuda())
    Xd = _shifted(X) if which == "X" else X.cuda()
    dYd = _shifted(dY) if which == "dY" else dY.cuda()
    off = 1 if which == "dG" else 0
    buf, dG = _guarded(R * I * O * S, dt, offset=off)
    h.ttm_grad_core(Xd, dYd, out=dG.view(R, I, O, S))
    assert torch.equal(dG, aligned.reshape(-1))
    assert _guards_intact(buf, R * I * O * S, offset=off)
    truth, bound = gc.grad_core_truth_and_bound(X, dY, dt)
    mc.assert_within(aligned, truth, bound, "ttm_grad_core {} {}".format(shape, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_grad_core_workspace_and_refusals_leave_the_output_untouched(dt):
    Lb = h.lib()
    code = h.dtype_code(dt)
    I, R, O, S = 3, 4, 2, 6
    L = h.ttm_grad_core_slab_rows(dt, I, 1, R, O, S)
    D1, D3 = 5, 2 * L + 7                                 # one slab, three slabs
    X1, _, dY1 = gc.grad_operands((I, D1, R, O, S), dt)
    X3, _, dY3 = gc.grad_operands((I, D3, R, O, S), dt)
    X1, dY1, X3, dY3 = X1.cuda(), dY1.cuda(), X3.cuda(), dY3.cuda()
    need = h.ttm_grad_core_workspace_bytes(dt, I, D3, R, O, S)
    assert need == 3 * I * R * O * S * X3.element_size() and h.ttm_grad_core_workspace_bytes(dt, I, D1, R, O, S) == 0
    ws = torch.empty(need, dtype=torch.uint8).cuda()
    buf, dG = _guarded(R * I * O * S, dt)
    before = buf.clone()

    def call(dtype=code, I=I, D=D1, R=R, O=O, S=S, x=X1, dy=dY1, dg=dG, w=None, wb=0):
        return Lb.ttr_ttm_grad_core(dtype, I, D, R, O, S, _ptr(x), _ptr(dy), _ptr(dg), _ptr(w), wb, None)

    assert call(D=D3, x=X3, dy=dY3, w=ws, wb=need - 1) == h.E_WORKSPACE      # one byte short
    assert call(D=D3, x=X3, dy=dY3, w=None, wb=need) == h.E_WORKSPACE        # several slabs need one
    assert call(dg=X1) == h.E_INVALID and call(dg=dY1) == h.E_INVALID         # the output is one of the inputs
    assert call(dtype=7) == h.E_INVALID
    for name in ("I", "D", "R", "O", "S"):
        assert call(**{name: 0}) == h.E_INVALID, name
    assert call(x=None) == h.E_INVALID and call(dy=None) == h.E_INVALID and call(dg=None) == h.E_INVALID
    assert call(D=2 ** 31) == h.E_UNSUPPORTED
    assert call(I=2 ** 16, R=2 ** 15) == h.E_UNSUPPORTED
    assert call(O=2 ** 16, S=2 ** 15) == h.E_UNSUPPORTED
    for query in (Lb.ttr_ttm_grad_core_slab_rows, Lb.ttr_ttm_grad_core_workspace_bytes):
        assert query(7, I, D1, R, O, S) == h.E_INVALID and query(code, I, 0, R, O, S) == h.E_INVALID
        assert query(code, I, 2 ** 31, R, O, S) == h.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    assert call() == 0                                    # one slab: a null workspace is fine
    torch.cuda.synchronize()
    truth, bound = gc.grad_core_truth_and_bound(X1, dY1, dt)
    mc.assert_within(dG.view(R, I, O, S), truth, bound, "one slab, null workspace {}".format(dt))
    assert call(D=D3, x=X3, dy=dY3, w=ws, wb=need) == 0   # exactly enough
    torch.cuda.synchronize()
    truth, bound = gc.grad_core_truth_and_bound(X3, dY3, dt)
    mc.assert_within(dG.view(R, I, O, S), truth, bound, "three slabs {}".format(dt))
    assert _guards_intact(buf, R * I * O * S)
    with pytest.raises(ValueError):
        h.ttm_grad_core(X1.permute(1, 0, 2).contiguous().permute(1, 0, 2), dY1)   # the binding refuses what the entry cannot express


def test_entries_are_exported():
    for name in ("ttr_ttm_grad_input", "ttr_ttm_grad_core_slab_rows", "ttr_ttm_grad_core_workspace_bytes", "ttr_ttm_grad_core"):
        assert name in h.EXPORTED_SYMBOLS and hasattr(h.lib(), name)

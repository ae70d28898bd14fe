"""``ttr_ttm_lookup_grad_core``, ``ttr_ttm_lookup_grad_input`` and ``ttr_segment_sum`` on a real MI355X, through the binding, in
fp32 and fp64: every shape of ``lookup_cases.STEP_SHAPES`` within the derived bounds of ``embedding_cases``; exact zeros in the
slices nobody asked for; the same bits on a second call, with the identity row map, from an unaligned output, for a row alone
and for a strided core; slices of several slabs; the segment lengths and widths of ``embedding_cases``; and the refusals of the
three entries, each with the output left as it was."""
import ctypes

import pytest
import torch

import embedding_cases as ec
import lookup_cases as lc
import matrix_cases as mc
from tntorch_amd import _hip

pytestmark = pytest.mark.gpu

DTYPES = ec.DTYPES
SENTINEL = -7.5


def _flag(value=0):
    return torch.full((1,), value, dtype=torch.int32, device="cuda")


def _perm(idx, I):
    """The sample ids grouped by wrapped index, stable; and the contiguous int64 index vector, both on the device."""
    idx = idx.cuda().long().contiguous()
    return idx, torch.sort(torch.remainder(idx, I), stable=True).indices


def _core(X, xrow, dY, idx, I, out=None, flag=None):
    R, (O, S) = X.shape[2], dY.shape[2:]
    idx, perm = _perm(idx, I)
    flag = _flag() if flag is None else flag
    out = torch.full((R, I, O, S), SENTINEL, dtype=X.dtype, device="cuda") if out is None else out
    xr = None if xrow is None else xrow.cuda().long().contiguous()
    _hip.ttm_lookup_grad_core(X, xr, dY, idx, perm, flag, out)
    return out, int(flag.item())


def _input(dY, G, idx, flag=None, out=None):
    idx, perm = _perm(idx, G.shape[1])
    flag = _flag() if flag is None else flag
    dX = _hip.ttm_lookup_grad_input(dY, G, idx, perm, flag, out=out)
    return dX, int(flag.item())


def _slab_rows(shape, dt):
    return _hip.ttm_lookup_grad_core_slab_rows(dt, *shape)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", lc.STEP_SHAPES)
def test_grad_core_every_shape(shape, dt):
    P, D, R, I, O, S = shape
    X, _, idx, dY = ec.grad_operands(shape, dt)
    Xd, dYd = X.cuda(), dY.cuda()
    dG, flag = _core(Xd, None, dYd, idx, I)
    assert flag == 0 and dG.dtype == dt
    dG64, bound, cnt = ec.grad_core_truth_and_bound(X, None, dY, idx, I, _slab_rows(shape, dt), dt)
    mc.assert_within(dG, dG64, bound, "lookup grad_core {} {}".format(shape, dt))
    assert bool((dG[:, (cnt == 0).cuda()] == 0).all())                                 # exact zeros where nobody asked
    dG2, _ = _core(Xd, None, dYd, idx, I)
    assert torch.equal(dG, dG2)                                                        # two calls
    dG3, flag = _core(Xd, torch.arange(P), dYd, idx, I)
    assert flag == 0 and torch.equal(dG, dG3)                                          # NULL and the identity row map
    buf = torch.full((dG.numel() + 1,), SENTINEL, dtype=dt, device="cuda")
    off1 = buf[1:].view(R, I, O, S)                                                    # one element off a 16-byte boundary
    assert off1.data_ptr() % 16 != 0
    _core(Xd, None, dYd, idx, I, out=off1)
    assert torch.equal(dG, off1) and float(buf[0]) == SENTINEL


def test_some_slices_have_several_slabs():
    """The slab rule's floor is low enough for the shapes of ``STEP_SHAPES`` to cut a slice: the partial tiles and the second
    launch's sum in slab order are what ``test_grad_core_every_shape`` checks there."""
    cut = []
    for shape in lc.STEP_SHAPES:
        P, D, R, I, O, S = shape
        _, _, idx, _ = ec.grad_operands(shape, torch.float32)
        cnt = torch.bincount(ec.wrapped(idx, I), minlength=I)
        rows = _slab_rows(shape, torch.float32)
        assert rows == _slab_rows(shape, torch.float64) and rows % 32 == 0
        if int((-(-cnt * D // rows)).max()) >= 2:
            cut.append(shape)
    print("slices of two or more slabs:", cut)
    assert len(cut) >= 2 and (65, 65, 33, 5, 5, 16) in cut and (300, 17, 3, 5, 1, 1) in cut


@pytest.mark.parametrize("dt", DTYPES)
def test_grad_core_row_map_and_one_slice(dt):
    shape = (300, 3, 33, 5, 15, 1)
    P, D, R, I, O, S = shape
    X, _, idx, dY = ec.grad_operands(shape, dt, rows_x=7)
    g = torch.Generator().manual_seed(2)
    xrow = torch.randint(0, 7, (P,), generator=g)
    for name, ix in (("row map", idx), ("one slice", torch.full((P,), 3)), ("negative", torch.randint(-I, 0, (P,), generator=g))):
        dG, flag = _core(X.cuda(), xrow, dY.cuda(), ix, I)
        dG64, bound, cnt = ec.grad_core_truth_and_bound(X, xrow, dY, ix, I, _slab_rows(shape, dt), dt)
        assert flag == 0
        mc.assert_within(dG, dG64, bound, "{} {}".format(name, dt))
        assert bool((dG[:, (cnt == 0).cuda()] == 0).all())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", lc.STEP_SHAPES)
def test_grad_input_every_shape(shape, dt):
    P, D, R, I, O, S = shape
    _, G, idx, dY = ec.grad_operands(shape, dt)
    Gd, dYd = G.cuda(), dY.cuda()
    dX, flag = _input(dYd, Gd, idx)
    assert flag == 0 and dX.dtype == dt and tuple(dX.shape) == (P, D, R)
    dX64, bound = ec.grad_input_truth_and_bound(dY, G, idx, dt)
    mc.assert_within(dX, dX64, bound, "lookup grad_input {} {}".format(shape, dt))
    for p in sorted({0, P // 2, P - 1}):                                               # a row's bits: the batch and the row alone
        one, flag = _input(dYd[p:p + 1].contiguous(), Gd, idx[p:p + 1])
        assert flag == 0 and torch.equal(one[0], dX[p])


@pytest.mark.parametrize("dt", DTYPES)
def test_grad_input_strides_of_G(dt):
    shape = (65, 3, 4, 5, 8, 8)
    P, D, R, I, O, S = shape
    _, G, idx, dY = ec.grad_operands(shape, dt)
    Gd, dYd = G.cuda(), dY.cuda()
    dX, _ = _input(dYd, Gd, idx)
    views = {
        "permuted": Gd.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3),
        "padded s": torch.cat([Gd, Gd[..., :3]], dim=3)[..., :S],
        "padded o": torch.cat([Gd, Gd[:, :, :1]], dim=2)[:, :, :O],
    }
    for name, V in views.items():
        assert not V.is_contiguous() and V.stride(3) == 1 and torch.equal(V, Gd)
        dXv, flag = _input(dYd, V, idx)
        assert flag == 0 and torch.equal(dXv, dX), name
    bad = torch.stack([Gd, Gd], dim=4)[..., 0]
    out = torch.full((P, D, R), SENTINEL, dtype=dt, device="cuda")
    with pytest.raises(NotImplementedError, match="unit stride"):
        _input(dYd, bad, idx, out=out)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


@pytest.mark.parametrize("dt", DTYPES)
def test_bad_indices_set_the_flag_and_write_nothing(dt):
    shape = (65, 3, 4, 5, 8, 8)
    P, D, R, I, O, S = shape
    X, G, idx, dY = ec.grad_operands(shape, dt)
    Xd, Gd, dYd = X.cuda(), G.cuda(), dY.cuda()
    bad = idx.clone()
    bad[17] = I
    good_idx, good_perm = _perm(idx, I)
    bad_perm = good_perm.clone()
    bad_perm[3] = P
    for ix, perm, word in ((bad.cuda(), good_perm, 0), (good_idx, bad_perm, 0), (good_idx, good_perm, 1)):
        flag = _flag(word)
        dG = torch.full((R, I, O, S), SENTINEL, dtype=dt, device="cuda")
        dX = torch.full((P, D, R), SENTINEL, dtype=dt, device="cuda")
        _hip.ttm_lookup_grad_core(Xd, None, dYd, ix, perm, flag, dG)
        _hip.ttm_lookup_grad_input(dYd, Gd, ix, perm, flag, out=dX)
        assert int(flag.item()) == 1 and bool((dG == SENTINEL).all()) and bool((dX == SENTINEL).all())
    flag = _flag()
    dG = torch.full((R, I, O, S), SENTINEL, dtype=dt, device="cuda")
    xrow = torch.arange(P, device="cuda")
    xrow[64] = P
    _hip.ttm_lookup_grad_core(Xd, xrow, dYd, good_idx, good_perm, flag, dG)
    assert int(flag.item()) == 1 and bool((dG == SENTINEL).all())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("C", ec.SEG_WIDTHS)
def test_segment_sum(C, dt):
    Y, w, perm, seg = ec.segment_operands(C, dt)
    Yd, wd, pd, sd = Y.cuda(), w.cuda(), perm.cuda(), seg.cuda()
    for ww, pp in ((None, None), (w, None), (None, perm), (w, perm)):
        args = dict(w=None if ww is None else wd, perm=None if pp is None else pd)
        out = _hip.segment_sum(Yd, sd, **args)
        assert out.dtype == dt and tuple(out.shape) == (len(ec.SEG_LENGTHS), C)
        out64, bound = ec.segment_truth_and_bound(Y, seg, ww, pp, dt)
        mc.assert_within(out, out64, bound, "segment_sum C = {} {} w {} perm {}".format(C, dt, ww is not None, pp is not None))
        assert bool((out[0] == 0).all()) and bool((out[-1] == 0).all())                # the empty segments
        assert torch.equal(out, _hip.segment_sum(Yd, sd, **args))                      # two calls
    if C % (16 // Y.element_size()) == 0:                                              # element loads from an unaligned Y: same bits
        buf = torch.empty(Y.numel() + 1, dtype=dt, device="cuda")
        off1 = buf[1:].view(Y.shape)
        off1.copy_(Yd)
        assert off1.data_ptr() % 16 != 0 and torch.equal(_hip.segment_sum(off1, sd, w=wd, perm=pd), out)
    # segments that leave rows out at both ends
    inner = sd[2:-2].contiguous()
    assert torch.equal(_hip.segment_sum(Yd, inner, w=wd, perm=pd), out[2:5])


def _raw(name, *args):
    p = lambda a: ctypes.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a
    return getattr(_hip.lib(), name)(*[p(a) for a in args], torch.cuda.current_stream().cuda_stream)


def test_refusals_before_any_launch():
    dt = torch.float32
    P, D, R, I, O, S = 5, 2, 3, 4, 2, 3
    X, G, idx, dY = ec.grad_operands((P, D, R, I, O, S), dt)
    X, G, dY = X.cuda(), G.cuda(), dY.cuda()
    idx, perm = _perm(idx, I)
    flag = _flag()
    code = _hip.dtype_code(dt)
    E_INVALID, E_UNSUPPORTED, E_WORKSPACE = _hip.E_INVALID, _hip.E_UNSUPPORTED, _hip.E_WORKSPACE

    # ---- ttr_ttm_lookup_grad_core
    dG = torch.full((R, I, O, S), SENTINEL, dtype=dt, device="cuda")
    wsb = _hip.ttm_lookup_grad_core_workspace_bytes(dt, P, D, R, I, O, S)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    base = dict(dtype=code, P=P, rows_x=P, D=D, R=R, I=I, O=O, S=S, X=X, xrow=None, dY=dY, idx=idx, stride=1, perm=perm, dG=dG,
                flag=flag, ws=ws, wsb=wsb)
    core = lambda **kw: _raw("ttr_ttm_lookup_grad_core", *{**base, **kw}.values())
    assert core() == 0
    torch.cuda.synchronize()
    assert int(flag.item()) == 0 and not bool((dG == SENTINEL).any())
    dG.fill_(SENTINEL)
    for name in ("X", "dY", "idx", "perm", "dG", "flag"):
        assert core(**{name: None}) == E_INVALID, name
    for name in ("rows_x", "D", "R", "I", "O", "S"):
        assert core(**{name: 0}) == E_INVALID, name
    assert core(dtype=7) == E_INVALID and core(P=-1) == E_INVALID and core(stride=0) == E_INVALID
    assert core(dG=X) == E_INVALID and core(dG=dY) == E_INVALID and core(ws=dY) == E_INVALID
    assert core(D=1 << 20, R=1 << 12) == E_UNSUPPORTED and core(O=1 << 20, S=1 << 12) == E_UNSUPPORTED
    assert core(ws=None) == E_WORKSPACE and core(wsb=wsb - 1) == E_WORKSPACE
    lib = _hip.lib()
    assert lib.ttr_ttm_lookup_grad_core_workspace_bytes(code, -1, D, R, I, O, S) == E_INVALID
    assert lib.ttr_ttm_lookup_grad_core_slab_rows(code, P, D, R, 0, O, S) == E_INVALID
    assert lib.ttr_ttm_lookup_grad_core_slab_rows(code, P, 1 << 20, 1 << 12, I, O, S) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert int(flag.item()) == 0 and bool((dG == SENTINEL).all())
    assert core(P=0, X=None, dY=None, idx=None, perm=None) == 0                      # no samples: zeros
    torch.cuda.synchronize()
    assert bool((dG == 0).all())

    # ---- ttr_ttm_lookup_grad_input
    dX = torch.full((P, D, R), SENTINEL, dtype=dt, device="cuda")
    wsb = _hip.ttm_lookup_grad_input_workspace_bytes(P, I)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    gs = (ctypes.c_int64 * 4)(*G.stride())
    base = dict(dtype=code, P=P, D=D, R=R, I=I, O=O, S=S, dY=dY, G=G, gs=gs, idx=idx, stride=1, perm=perm, dX=dX, flag=flag, ws=ws,
                wsb=wsb)
    inp = lambda **kw: _raw("ttr_ttm_lookup_grad_input", *{**base, **kw}.values())
    assert inp() == 0
    torch.cuda.synchronize()
    assert int(flag.item()) == 0 and not bool((dX == SENTINEL).any())
    dX.fill_(SENTINEL)
    for name in ("dY", "G", "gs", "idx", "perm", "dX", "flag"):
        assert inp(**{name: None}) == E_INVALID, name
    for name in ("D", "R", "I", "O", "S"):
        assert inp(**{name: 0}) == E_INVALID, name
    assert inp(dtype=7) == E_INVALID and inp(P=-1) == E_INVALID and inp(stride=0) == E_INVALID
    assert inp(dX=dY) == E_INVALID and inp(dX=G) == E_INVALID
    s = list(G.stride())
    assert inp(gs=(ctypes.c_int64 * 4)(s[0], s[1], s[2], 2)) == E_UNSUPPORTED
    assert inp(gs=(ctypes.c_int64 * 4)(-s[0], s[1], s[2], 1)) == E_UNSUPPORTED
    assert inp(D=1 << 20, R=1 << 12) == E_UNSUPPORTED and inp(O=1 << 20, S=1 << 12) == E_UNSUPPORTED
    assert inp(ws=None) == E_WORKSPACE and inp(wsb=wsb - 1) == E_WORKSPACE
    assert inp(P=0, dY=None, G=None, gs=None, idx=None, perm=None, dX=None, flag=None, ws=None, wsb=0) == 0
    assert lib.ttr_ttm_lookup_grad_input_workspace_bytes(-1, 4) < 0 and lib.ttr_ttm_lookup_grad_input_workspace_bytes(4, 0) < 0
    torch.cuda.synchronize()
    assert int(flag.item()) == 0 and bool((dX == SENTINEL).all())

    # ---- ttr_segment_sum
    B, C = 3, 6
    Y = torch.randn((P, C), dtype=dt, device="cuda")
    seg = torch.tensor([0, 2, 2, 5], device="cuda")
    out = torch.full((B, C), SENTINEL, dtype=dt, device="cuda")
    base = dict(dtype=code, B=B, P=P, C=C, Y=Y, w=None, perm=None, seg=seg, out=out)
    ssum = lambda **kw: _raw("ttr_segment_sum", *{**base, **kw}.values())
    for name in ("Y", "seg", "out"):
        assert ssum(**{name: None}) == E_INVALID, name
    assert ssum(dtype=7) == E_INVALID and ssum(B=-1) == E_INVALID and ssum(P=-1) == E_INVALID and ssum(C=0) == E_INVALID
    assert ssum(out=Y) == E_INVALID and ssum(out=seg) == E_INVALID
    assert ssum(P=1 << 40, C=1 << 20) == E_UNSUPPORTED
    assert ssum(B=0, Y=None, seg=None, out=None) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert ssum() == 0 and ssum(P=0, Y=None, out=out) == 0                             # no rows: every segment is empty
    torch.cuda.synchronize()
    assert bool((out == 0).all())
    # bounds outside 0 .. P and a row id outside 0 .. P - 1 are clamped / skipped, never read
    wild = torch.tensor([-3, 2, 1, 9], device="cuda")
    pm = torch.tensor([0, 1, 7, -1, 4], device="cuda")
    assert ssum(seg=wild, perm=pm) == 0
    torch.cuda.synchronize()
    want = torch.stack([Y[0] + Y[1], torch.zeros(C, device="cuda"), Y[1] + Y[4]])      # [0, 2), empty, [1, 5) without 7 and -1
    assert torch.allclose(out, want, rtol=1e-6, atol=1e-6)


def test_symbols_are_exported():
    lib = _hip.lib()
    for name in ("ttr_ttm_lookup_grad_core_slab_rows", "ttr_ttm_lookup_grad_core_workspace_bytes", "ttr_ttm_lookup_grad_core",
                 "ttr_ttm_lookup_grad_input_workspace_bytes", "ttr_ttm_lookup_grad_input", "ttr_segment_sum"):
        assert name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name)

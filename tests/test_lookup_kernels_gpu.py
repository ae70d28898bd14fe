"""``ttr_ttm_lookup_step`` on a real MI355X, through the binding, in fp32 and fp64: every shape of ``lookup_cases.STEP_SHAPES``
within the derived step bound; the index patterns (one group of many tiles, all distinct, unasked slices, negative indices, row
maps); that a row's bits depend on nothing but its own operands (permutation, subset, NULL against identity row map, two calls);
the strides of G; and the refusals, each with Y left as it was."""
import ctypes

import pytest
import torch

import lookup_cases as lc
import matrix_cases as mc
from tntorch_amd import _hip

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
SENTINEL = -7.5


def _flag(value=0):
    return torch.full((1,), value, dtype=torch.int32, device="cuda")


def _run(X, xrow, G, idx, flag=None, out=None):
    """(Y, flag word) of one call; idx / xrow are moved to the device as contiguous int64 vectors."""
    flag = _flag() if flag is None else flag
    xr = None if xrow is None else xrow.cuda().long().contiguous()
    Y = _hip.ttm_lookup_step(X, xr, G, idx.cuda().long().contiguous(), flag, out=out)
    return Y, int(flag.item())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", lc.STEP_SHAPES)
def test_every_shape_within_the_step_bound(shape, dt):
    X, G, idx = lc.step_operands(shape, dt)
    Y, flag = _run(X.cuda(), None, G.cuda(), idx)
    assert flag == 0 and Y.is_cuda and Y.dtype == dt and tuple(Y.shape) == (shape[0], shape[1], shape[4], shape[5])
    Y64, bound = lc.step_truth_and_bound(X, None, G, idx, dt)
    mc.assert_within(Y, Y64, bound, "lookup step {} {}".format(shape, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_index_patterns(dt):
    shape = (300, 3, 33, 5, 15, 1)
    P, I = shape[0], shape[3]
    X, G, idx = lc.step_operands(shape, dt)
    Xd, Gd = X.cuda(), G.cuda()
    g = torch.Generator().manual_seed(2)
    patterns = {
        "one slice": torch.full((P,), 3),                                   # one group of ceil(900 / 64) tiles
        "unasked slices": torch.tensor([1, 3])[torch.randint(0, 2, (P,), generator=g)],
        "negative": torch.randint(-I, 0, (P,), generator=g),
    }
    for name, ix in patterns.items():
        Y, flag = _run(Xd, None, Gd, ix)
        Y64, bound = lc.step_truth_and_bound(X, None, G, ix, dt)
        assert flag == 0
        mc.assert_within(Y, Y64, bound, "{} {}".format(name, dt))
    # a row map with repeats into fewer X rows
    Xs = X[:7].contiguous()
    xrow = torch.randint(0, 7, (P,), generator=g)
    Y, flag = _run(Xs.cuda(), xrow, Gd, idx)
    Y64, bound = lc.step_truth_and_bound(Xs, xrow, G, idx, dt)
    assert flag == 0
    mc.assert_within(Y, Y64, bound, "row map {}".format(dt))
    # NULL and the identity row map: the same bits
    Y0, _ = _run(Xd, None, Gd, idx)
    Y1, flag = _run(Xd, torch.arange(P), Gd, idx)
    assert flag == 0 and torch.equal(Y0, Y1)
    # all distinct, on a mode beyond the LDS histogram bins
    shape = (300, 1, 4, 1025, 1, 1)
    X, G, _ = lc.step_operands(shape, dt)
    ix = torch.randperm(1025, generator=g)[:300]
    Y, flag = _run(X.cuda(), None, G.cuda(), ix)
    Y64, bound = lc.step_truth_and_bound(X, None, G, ix, dt)
    assert flag == 0
    mc.assert_within(Y, Y64, bound, "all distinct {}".format(dt))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", [(300, 3, 33, 5, 15, 1), (65, 17, 1, 1025, 3, 5), (65, 65, 33, 5, 5, 16)])
def test_a_rows_bits_are_its_own(shape, dt):
    P = shape[0]
    X, G, idx = lc.step_operands(shape, dt)
    Xd, Gd = X.cuda(), G.cuda()
    Y, _ = _run(Xd, None, Gd, idx)
    Y2, _ = _run(Xd, None, Gd, idx)
    assert torch.equal(Y, Y2)                                               # two calls
    g = torch.Generator().manual_seed(4)
    perm = torch.randperm(P, generator=g)
    Yp, flag = _run(Xd, perm, Gd, idx[perm])                                # sample p' is sample perm[p']
    assert flag == 0 and torch.equal(Yp, Y[perm.cuda()])
    sub = perm[:max(1, P // 5)]
    Ys, flag = _run(Xd, sub, Gd, idx[sub])                                  # fewer samples, other groups, other tiles
    assert flag == 0 and torch.equal(Ys, Y[sub.cuda()])
    Y1, flag = _run(Xd[sub[:1]].contiguous(), None, Gd, idx[sub[:1]])       # one sample alone
    assert flag == 0 and torch.equal(Y1[0], Y[sub[0]])


@pytest.mark.parametrize("dt", DTYPES)
def test_strides_of_G(dt):
    shape = (65, 3, 4, 5, 8, 8)
    P, D, R, I, O, S = shape
    X, G, idx = lc.step_operands(shape, dt)
    Xd, Gd = X.cuda(), G.cuda()
    Y, _ = _run(Xd, None, Gd, idx)
    views = {
        "permuted": Gd.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3),                       # [I, R, O, S] underneath
        "padded s": torch.cat([Gd, Gd[..., :3]], dim=3)[..., :S],                                  # o stride S + 3
        "padded o": torch.cat([Gd, Gd[:, :, :1]], dim=2)[:, :, :O],                                # i stride (O + 1) S
    }
    for name, V in views.items():
        assert not V.is_contiguous() and V.stride(3) == 1 and torch.equal(V, Gd)
        Yv, flag = _run(Xd, None, V, idx)
        assert flag == 0 and torch.equal(Yv, Y), name
    bad = torch.stack([Gd, Gd], dim=4)[..., 0]                                                     # last stride 2
    assert bad.stride(3) == 2
    out = torch.full((P, D, O, S), SENTINEL, dtype=dt, device="cuda")
    with pytest.raises(NotImplementedError, match="unit stride"):
        _run(Xd, None, bad, idx, out=out)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


@pytest.mark.parametrize("dt", DTYPES)
def test_bad_indices_set_the_flag_and_write_nothing(dt):
    shape = (65, 3, 4, 5, 8, 8)
    P, D, R, I, O, S = shape
    X, G, idx = lc.step_operands(shape, dt)
    Xd, Gd = X.cuda(), G.cuda()
    ident = torch.arange(P)

    def poisoned(v, at, value):
        v = v.clone()
        v[at] = value
        return v

    cases = [(None, poisoned(idx, 17, I)), (None, poisoned(idx, 0, -I - 1)), (poisoned(ident, 64, P), idx),
             (poisoned(ident, 3, -1), idx)]
    for xrow, ix in cases:
        out = torch.full((P, D, O, S), SENTINEL, dtype=dt, device="cuda")
        _, flag = _run(Xd, xrow, Gd, ix, out=out)
        assert flag == 1 and bool((out == SENTINEL).all())
    # a word that is set on entry: nothing is written, and the word stays
    out = torch.full((P, D, O, S), SENTINEL, dtype=dt, device="cuda")
    _, flag = _run(Xd, None, Gd, idx, flag=_flag(1), out=out)
    assert flag == 1 and bool((out == SENTINEL).all())
    # the word is not cleared by a good call either: a chain shares it
    word = _flag()
    _run(Xd, None, Gd, poisoned(idx, 5, I), flag=word, out=out)
    _, flag = _run(Xd, None, Gd, idx, flag=word, out=out)
    assert flag == 1 and bool((out == SENTINEL).all())


def _raw(dt, P, rows_x, D, R, I, O, S, X, xrow, G, gs, idx, stride, Y, flag, ws, wsb):
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    strides = None if gs is None else (ctypes.c_int64 * 4)(*gs)
    return _hip.lib().ttr_ttm_lookup_step(_hip.dtype_code(dt), P, rows_x, D, R, I, O, S, p(X), p(xrow), p(G), strides, p(idx), stride,
                                          p(Y), p(flag), p(ws), wsb, torch.cuda.current_stream().cuda_stream)


def test_refusals_before_any_launch():
    dt = torch.float32
    P, D, R, I, O, S = 5, 2, 3, 4, 2, 3
    X, G, idx = lc.step_operands((P, D, R, I, O, S), dt)
    X, G, idx = X.cuda(), G.cuda(), idx.cuda()
    Y = torch.full((P, D, O, S), SENTINEL, dtype=dt, device="cuda")
    flag = _flag()
    wsb = _hip.ttm_lookup_workspace_bytes(P, I)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    gs = list(G.stride())
    args = dict(X=X, xrow=None, G=G, gs=gs, idx=idx, stride=1, Y=Y, flag=flag, ws=ws, wsb=wsb)
    call = lambda P_=P, rows_x=P, D_=D, R_=R, I_=I, O_=O, S_=S, **kw: _raw(dt, P_, rows_x, D_, R_, I_, O_, S_, **{**args, **kw})
    assert call() == 0
    torch.cuda.synchronize()
    assert int(flag.item()) == 0 and not bool((Y == SENTINEL).any())
    Y.fill_(SENTINEL)
    for name in ("X", "G", "gs", "idx", "Y", "flag"):
        assert call(**{name: None}) == _hip.E_INVALID, name
    for name in ("rows_x", "D_", "R_", "I_", "O_", "S_"):
        assert call(**{name: 0}) == _hip.E_INVALID, name
    assert call(P_=-1) == _hip.E_INVALID and call(stride=0) == _hip.E_INVALID
    assert call(Y=X) == _hip.E_INVALID and call(Y=G) == _hip.E_INVALID
    lib = _hip.lib()
    assert lib.ttr_ttm_lookup_step(7, P, P, D, R, I, O, S, None, None, None, None, None, 1, None, None, None, 0, None) == _hip.E_INVALID
    assert call(gs=[gs[0], gs[1], gs[2], 2]) == _hip.E_UNSUPPORTED and call(gs=[-gs[0], gs[1], gs[2], 1]) == _hip.E_UNSUPPORTED
    assert call(D_=1 << 20, R_=1 << 12) == _hip.E_UNSUPPORTED and call(O_=1 << 20, S_=1 << 12) == _hip.E_UNSUPPORTED
    assert call(ws=None) == _hip.E_WORKSPACE and call(wsb=wsb - 1) == _hip.E_WORKSPACE
    # P = 0 touches nothing, whatever the pointers
    assert lib.ttr_ttm_lookup_step(_hip.F32, 0, 1, D, R, I, O, S, None, None, None, None, None, 1, None, None, None, 0, None) == 0
    torch.cuda.synchronize()
    assert int(flag.item()) == 0 and bool((Y == SENTINEL).all())
    assert tuple(_hip.ttm_lookup_step(X[:0], None, G, idx[:0], flag).shape) == (0, D, O, S)
    assert lib.ttr_ttm_lookup_workspace_bytes(-1, 4) < 0 and lib.ttr_ttm_lookup_workspace_bytes(4, 0) < 0
    assert lib.ttr_ttm_lookup_workspace_bytes(0, 1) > 0


def test_symbols_are_exported():
    lib = _hip.lib()
    for name in ("ttr_ttm_lookup_workspace_bytes", "ttr_ttm_lookup_step"):
        assert name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name)

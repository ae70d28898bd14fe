"""``tn.tt_embedding`` and ``tn.tt_embedding_bag`` on a real MI355X: values and the gradients of the cores against autograd
through the dense fp64 matrix within the derived bounds of ``embedding_cases`` (every form of a bag, every single core requiring
grad and all of them, frozen cores without a gradient); the forward's bits against ``tt_lookup``; the launches of the backward;
that the backward reads nothing back; the refusals; and one optimizer step."""
import functools

import pytest
import torch

import embedding_cases as ec
import lookup_cases as lc
import matrix_cases as mc
import tntorch_amd as tn
from tntorch_amd import _hip

pytestmark = pytest.mark.gpu

DTYPES = ec.DTYPES
NAMES = ec.NAMES
FORMS = [None] + ec.BAG_FORMS
FORM_IDS = ["embedding"] + [f[0] for f in ec.BAG_FORMS]


def _operands(name, form, dt):
    """(cores on the CPU, idims, odims, ncols, rows, offsets, weights, mode, seg, cotangent): CPU tensors, fp64 cotangent."""
    tt, idims, odims, nrows, ncols = ec.case(name, dt)
    if form is None:
        rows, offsets, w, mode, seg = lc.lookup_rows(nrows), None, None, "sum", None
        g = ec.cotangent((2, 6, ncols))
    else:
        rows, offsets, w, mode, seg = ec.bag_operands(form, nrows, dt)
        g = ec.cotangent((len(seg) - 1, ncols))
    return tt, idims, odims, ncols, rows, offsets, w, mode, seg, g


@functools.lru_cache(maxsize=None)
def _reference(name, form_id, dt):
    """The fp64 truth of a case, computed once and shared: (value, its magnitude, core gradients, their magnitudes)."""
    tt, idims, odims, ncols, rows, offsets, w, mode, seg, g = _operands(name, FORMS[FORM_IDS.index(form_id)], dt)
    y64, grads = ec.reference(tt, rows, seg, w, mode, g.to(dt))
    ymag, gmags = ec.reference(tt, rows, seg, w, mode, g.to(dt), magnitudes=True)
    return y64, ymag, grads, gmags


def _call(cores, idims, odims, form, rows, offsets, w, mode):
    ttm = tn.TTMatrix(cores, None, idims, odims)
    dev = lambda t: None if t is None else t.cuda()
    if form is None:
        return tn.tt_embedding(ttm, rows.cuda())
    return tn.tt_embedding_bag(ttm, rows.cuda(), dev(offsets), dev(w), mode)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("name", NAMES)
def test_values_and_gradients(name, form, dt):
    tt, idims, odims, ncols, rows, offsets, w, mode, seg, g = _operands(name, form, dt)
    y64, ymag, grads64, gmags = _reference(name, "embedding" if form is None else form[0], dt)
    d, u = len(tt), mc.unit(dt)
    slab_rows = lambda k, P, D: _hip.ttm_lookup_grad_core_slab_rows(dt, P, D, tt[k].shape[0], tt[k].shape[1], tt[k].shape[2], tt[k].shape[3])
    consts = ec.grad_constants(tt, idims, rows, seg, slab_rows)
    what = "{} {} {}".format(name, "embedding" if form is None else form[0], dt)
    gd = g.to(dt).cuda()
    for live in [[k] for k in range(d)] + ([list(range(d))] if d > 1 else []):          # each single core, and all of them
        cores = [c.cuda().requires_grad_(k in live) for k, c in enumerate(tt)]
        y = _call(cores, idims, odims, form, rows, offsets, w, mode)
        assert y.is_cuda and y.dtype == dt and y.requires_grad and tuple(y.shape) == tuple(y64.shape)
        mc.assert_within(y, y64, 2 * ec.value_constant(tt, seg) * u * ymag, "value " + what)
        y.backward(gd)
        for k, c in enumerate(cores):
            if k not in live:
                assert c.grad is None                                               # a frozen core gets no gradient
                continue
            assert c.grad.is_cuda and c.grad.dtype == dt and c.grad.shape == c.shape
            mc.assert_within(c.grad, grads64[k], 2 * consts[k] * u * gmags[k], "dG_{} (live {}) {}".format(k, live, what))
    if seg is not None and offsets is not None:
        assert bool((y[0] == 0).all()) and bool((y[2] == 0).all()) and bool((y[5] == 0).all())   # the empty bags


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_forward_bits_and_tt_lookup_still_refuses(name, dt):
    tt, idims, odims, ncols, rows, _, _, _, _, _ = _operands(name, None, dt)
    rows = rows.cuda()
    frozen = tn.TTMatrix([c.cuda() for c in tt], None, idims, odims)
    want = tn.tt_lookup(frozen, rows)
    assert torch.equal(tn.tt_embedding(frozen, rows), want)                             # no core requires grad
    cores = [c.cuda().requires_grad_(True) for c in tt]
    live = tn.TTMatrix(cores, None, idims, odims)
    with torch.no_grad():
        y = tn.tt_embedding(live, rows)
    assert not y.requires_grad and torch.equal(y, want)
    y = tn.tt_embedding(live, rows)                                                     # the recorded forward: the same bits
    assert y.requires_grad and torch.equal(y.detach(), want)
    for r in (rows.int(), rows.tolist(), rows.cpu().numpy()):
        assert torch.equal(tn.tt_embedding(live, r).detach(), want)
    with pytest.raises(NotImplementedError, match="tt_lookup is not differentiable on the device"):
        tn.tt_lookup(live, rows)
    # a bag of one row each is the row, in every mode
    flat = rows.reshape(-1)
    offsets = torch.arange(flat.numel(), device="cuda")
    for mode in ("sum", "mean"):
        assert torch.equal(tn.tt_embedding_bag(live, flat, offsets, mode=mode).detach(), want.reshape(flat.numel(), ncols))


def _count_calls(monkeypatch):
    calls = []
    real = _hip._call

    def counting(name, *args):
        calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(_hip, "_call", counting)
    return calls


def test_launch_counts(monkeypatch):
    """The forward is ``tt_lookup``'s launches (+ one segment sum for the bags).  The backward launches one grad_core per core
    k >= 2 that requires grad, one grad_input per step with a core before it that does, and one segment sum for the first core:
    for ``three`` with every core live that is two grad_core, TWO grad_input (dZ_2 for the second core, dZ_1 for the first: the
    first core's gradient is the segment sum OF dZ_1) and one segment sum."""
    calls = _count_calls(monkeypatch)
    step, core, inp, ssum = "ttr_ttm_lookup_step", "ttr_ttm_lookup_grad_core", "ttr_ttm_lookup_grad_input", "ttr_segment_sum"
    cases = [
        ("three", [0, 1, 2], [step] * 2, [core, inp, core, inp, ssum]),
        ("three", [1, 2], [step] * 2, [core, inp, core]),                              # the chain ends where nothing earlier needs one
        ("three", [2], [step] * 2, [core]),
        ("three", [1], [step] * 2, [inp, core]),
        ("three", [0], [step] * 2, [inp, inp, ssum]),
        ("ref", [0, 1], [step], [core, inp, ssum]),
        ("single", [0], [], [ssum]),
    ]
    for name, live, fwd, bwd in cases:
        tt, idims, odims, ncols, rows, _, _, _, _, g = _operands(name, None, torch.float32)
        cores = [c.cuda().requires_grad_(k in live) for k, c in enumerate(tt)]
        gd = g.float().cuda()
        del calls[:]
        y = tn.tt_embedding(tn.TTMatrix(cores, None, idims, odims), rows.cuda())
        assert calls == fwd, (name, live)
        del calls[:]
        y.backward(gd)
        assert calls == bwd, (name, live)
        del calls[:]
        yb = tn.tt_embedding_bag(tn.TTMatrix(cores, None, idims, odims), rows.cuda(), mode="mean")
        assert calls == fwd + [ssum], (name, live)
        del calls[:]
        yb.backward(torch.ones_like(yb))
        assert calls == bwd, (name, live)
    # frozen cores: tt_lookup's launches and nothing else
    tt, idims, odims, _, rows, _, _, _, _, _ = _operands("three", None, torch.float32)
    del calls[:]
    tn.tt_embedding(tn.TTMatrix([c.cuda() for c in tt], None, idims, odims), rows.cuda())
    assert calls == [step] * 2


@pytest.mark.parametrize("form", [None, ec.BAG_FORMS[5]], ids=["embedding", "offsets-weights"])
def test_backward_reads_nothing_back(form, monkeypatch):
    """No host synchronisation in the backward: under torch's sync debug mode where the build has it, and with ``item``, ``cpu``,
    ``tolist`` and ``numpy`` patched to raise in any case."""
    tt, idims, odims, ncols, rows, offsets, w, mode, seg, g = _operands("three", form, torch.float32)
    cores = [c.cuda().requires_grad_(True) for c in tt]
    y = _call(cores, idims, odims, form, rows, offsets, w, mode)
    gd = g.float().cuda()
    torch.cuda.synchronize()

    def refuse(*args, **kwargs):
        raise AssertionError("the backward read from the device")

    try:
        torch.cuda.set_sync_debug_mode("error")
        debug = True
    except Exception:   # (a build without the mode)
        debug = False
    try:
        with monkeypatch.context() as m:
            for method in ("item", "cpu", "tolist", "numpy"):
                m.setattr(torch.Tensor, method, refuse)
            y.backward(gd)
    finally:
        if debug:
            torch.cuda.set_sync_debug_mode("default")
    print("sync debug mode:", debug)
    assert all(c.grad is not None and bool(torch.isfinite(c.grad).all()) for c in cores)


def test_refusals_on_the_device():
    tt, idims, odims, ncols, rows, _, _, _, _, _ = _operands("three", None, torch.float64)
    cores = [c.cuda().requires_grad_(True) for c in tt]
    ttm = tn.TTMatrix(cores, None, idims, odims)
    rows = rows.cuda()
    flat, off = rows.reshape(-1), torch.tensor(ec.OFFSETS).cuda()
    w = torch.ones(12, dtype=torch.float64, device="cuda")
    nrows = 60
    for call in (lambda r: tn.tt_embedding(ttm, r), lambda r: tn.tt_embedding_bag(ttm, r)):
        with pytest.raises(ValueError, match="same device"):
            call(rows.cpu())
        with pytest.raises(ValueError, match="int32 or int64"):
            call(rows.double())
        for bad in (nrows, -nrows - 1):
            with pytest.raises(IndexError, match="outside the matrix"):
                call(torch.tensor([[0, bad, 1]]).cuda())
    with pytest.raises(ValueError, match="mode must be"):
        tn.tt_embedding_bag(ttm, rows, mode="max")
    with pytest.raises(ValueError, match="take no offsets"):
        tn.tt_embedding_bag(ttm, rows, off)
    with pytest.raises(ValueError, match="need the offsets"):
        tn.tt_embedding_bag(ttm, flat)
    with pytest.raises(ValueError, match="1-D .* or 2-D"):
        tn.tt_embedding_bag(ttm, rows[None])
    with pytest.raises(ValueError, match="offsets must be a 1-D int32 or int64"):
        tn.tt_embedding_bag(ttm, flat, off.double())
    with pytest.raises(ValueError, match="offsets must be on the same device"):
        tn.tt_embedding_bag(ttm, flat, off.cpu())
    for bad in ([0, 5, 3], [1, 3], [0, 13]):
        with pytest.raises(ValueError, match="offsets must start at 0"):
            tn.tt_embedding_bag(ttm, flat, torch.tensor(bad).cuda())
    for bad in (w[:11], w.float(), w.cpu()):
        with pytest.raises(ValueError, match="per_sample_weights must be"):
            tn.tt_embedding_bag(ttm, flat, off, bad)
    with pytest.raises(ValueError, match="mode 'sum' only"):
        tn.tt_embedding_bag(ttm, flat, off, w, "mean")
    wl = w.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="gradient of per_sample_weights"):
        tn.tt_embedding_bag(ttm, flat, off, wl)
    with torch.no_grad():
        assert tuple(tn.tt_embedding_bag(ttm, flat, off, wl).shape) == (6, ncols)
    # empty rows
    none = torch.zeros((0,), dtype=torch.int64, device="cuda")
    assert tuple(tn.tt_embedding(ttm, none).shape) == (0, ncols)
    y = tn.tt_embedding_bag(ttm, none, torch.zeros(3, dtype=torch.int64, device="cuda"))
    assert y.is_cuda and tuple(y.shape) == (3, ncols) and bool((y == 0).all())


def test_one_sgd_step_moves_every_core():
    tt, idims, odims, ncols, rows, _, _, _, _, _ = _operands("three", None, torch.float32)
    params = [torch.nn.Parameter(c.cuda()) for c in tt]
    before = [p.detach().clone() for p in params]
    opt = torch.optim.SGD(params, lr=0.1)
    opt.zero_grad()
    out = tn.tt_embedding_bag(tn.TTMatrix(params, None, idims, odims), rows.cuda(), mode="mean")
    loss = (out ** 2).sum()
    loss.backward()
    opt.step()
    for p, b in zip(params, before):
        assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), b)

"""``tn.tt_embedding`` and ``tn.tt_embedding_bag`` on the CPU (plain torch over the host chain): values against the dense fp64
truth within the derived bounds, every argument form and refusal, empty bags and rows, the gradients of the cores against
autograd through the dense matrix, the three host mirrors of the new kernels against autograd, and the wiring of the feature."""
import os
import re

import numpy as np
import pytest
import torch

import embedding_cases as ec
import lookup_cases as lc
import matrix_cases as mc
import tntorch_amd as tn
from tntorch_amd import _hip, _hipops, _hostops

DTYPES = ec.DTYPES
NAMES = ec.NAMES


def _matrix(name, dt):
    tt, idims, odims, nrows, ncols = ec.case(name, dt)
    return tn.TTMatrix(tt, None, idims, odims), tt, nrows, ncols


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_embedding_on_the_host(name, dt):
    ttm, tt, nrows, ncols = _matrix(name, dt)
    rows = lc.lookup_rows(nrows)
    y64, bound = lc.truth_and_bound(tt, rows, dt)
    y = tn.tt_embedding(ttm, rows)
    assert y.device.type == "cpu" and y.dtype == dt and tuple(y.shape) == (2, 6, ncols)
    mc.assert_within(y, y64, bound, "tt_embedding {} {}".format(name, dt))
    assert torch.equal(y, tn.tt_lookup(ttm, rows))
    flat = rows.reshape(-1)
    for r in (flat, flat.int(), flat.tolist(), tuple(flat.tolist()), flat.numpy()):
        assert torch.equal(tn.tt_embedding(ttm, r), y.reshape(12, ncols))
    for empty in (torch.zeros((0,), dtype=torch.int64), torch.zeros((3, 0), dtype=torch.int32), []):
        y0 = tn.tt_embedding(ttm, empty)
        assert y0.dtype == dt and tuple(y0.shape) == tuple(torch.as_tensor(empty).shape) + (ncols,)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("form", ec.BAG_FORMS, ids=[f[0] for f in ec.BAG_FORMS])
@pytest.mark.parametrize("name", NAMES)
def test_bags_on_the_host(name, form, dt):
    ttm, tt, nrows, ncols = _matrix(name, dt)
    rows, offsets, w, mode, seg = ec.bag_operands(form, nrows, dt)
    B = len(seg) - 1
    g = torch.zeros((B, ncols), dtype=torch.float64)
    y64, _ = ec.reference(tt, rows, seg, w, mode, g)
    mag, _ = ec.reference(tt, rows, seg, w, mode, g, magnitudes=True)
    y = tn.tt_embedding_bag(ttm, rows, offsets, w, mode)
    assert y.device.type == "cpu" and y.dtype == dt and tuple(y.shape) == (B, ncols)
    mc.assert_within(y, y64, 2 * ec.value_constant(tt, seg) * mc.unit(dt) * mag, "tt_embedding_bag {} {} {}".format(name, form[0], dt))
    if offsets is not None:
        assert bool((y[0] == 0).all()) and bool((y[2] == 0).all()) and bool((y[5] == 0).all())   # the empty bags
        for other in (offsets.int(), offsets.tolist()):
            assert torch.equal(tn.tt_embedding_bag(ttm, rows.tolist(), other, w, mode), y)


def test_empty_rows_and_no_bags_on_the_host():
    ttm, _, _, ncols = _matrix("three", torch.float64)
    none = torch.zeros((0,), dtype=torch.int64)
    y = tn.tt_embedding_bag(ttm, none, torch.tensor([0, 0, 0]))
    assert tuple(y.shape) == (3, ncols) and bool((y == 0).all())
    assert tuple(tn.tt_embedding_bag(ttm, none, none).shape) == (0, ncols)
    assert tuple(tn.tt_embedding_bag(ttm, torch.zeros((4, 0), dtype=torch.int64), mode="mean").shape) == (4, ncols)
    with pytest.raises(ValueError, match="offsets must start at 0"):
        tn.tt_embedding_bag(ttm, none, torch.tensor([0, 1]))


def test_refusals_on_the_host():
    ttm, tt, nrows, _ = _matrix("three", torch.float64)
    rows = lc.lookup_rows(nrows)
    flat, off = rows.reshape(-1), torch.tensor(ec.OFFSETS)
    w = torch.ones(12, dtype=torch.float64)
    for call in (lambda m, r: tn.tt_embedding(m, r), lambda m, r: tn.tt_embedding_bag(m, r)):
        with pytest.raises(ValueError, match="must be a TTMatrix"):
            call(tt, rows)
        with pytest.raises(ValueError, match="batched"):
            call(tn.TTMatrix([c[None] for c in tt], None, [4, 3, 5], [2, 6, 3]), rows)
        with pytest.raises(ValueError, match="boundary ranks"):
            call(tn.TTMatrix(tt[1:], None, [3, 5], [6, 3]), rows)
        with pytest.raises(ValueError, match="float32 or float64"):
            call(tn.TTMatrix([c.half() for c in tt], None, [4, 3, 5], [2, 6, 3]), rows)
        with pytest.raises(ValueError, match="same dtype"):
            call(tn.TTMatrix([tt[0], tt[1].float(), tt[2]], None, [4, 3, 5], [2, 6, 3]), rows)
        with pytest.raises(ValueError, match="same device"):
            call(ttm, rows.to("meta"))
        for bad in (rows.double(), rows > 0, [[0.5, 1.0]]):
            with pytest.raises(ValueError, match="int32 or int64"):
                call(ttm, bad)
        for bad in (nrows, -nrows - 1):
            with pytest.raises(IndexError, match="outside the matrix"):
                call(ttm, torch.tensor([[0, bad, 1]]))
    for mode in ("max", "prod", None):
        with pytest.raises(ValueError, match="mode must be"):
            tn.tt_embedding_bag(ttm, rows, mode=mode)
    with pytest.raises(ValueError, match="take no offsets"):
        tn.tt_embedding_bag(ttm, rows, off)
    with pytest.raises(ValueError, match="need the offsets"):
        tn.tt_embedding_bag(ttm, flat)
    for bad in (rows[None], torch.tensor(3)):
        with pytest.raises(ValueError, match="1-D .* or 2-D"):
            tn.tt_embedding_bag(ttm, bad)
    for bad in (off.double(), off[None], [0.0, 1.0]):
        with pytest.raises(ValueError, match="offsets must be a 1-D int32 or int64"):
            tn.tt_embedding_bag(ttm, flat, bad)
    with pytest.raises(ValueError, match="offsets must be on the same device"):
        tn.tt_embedding_bag(ttm, flat, off.to("meta"))
    for bad in ([0, 5, 3], [1, 3], [0, 13], [-1, 3]):
        with pytest.raises(ValueError, match="offsets must start at 0"):
            tn.tt_embedding_bag(ttm, flat, torch.tensor(bad))
    for bad in (w[:11], w.float(), w.to("meta"), w.tolist()):
        with pytest.raises(ValueError, match="per_sample_weights must be"):
            tn.tt_embedding_bag(ttm, flat, off, bad)
    with pytest.raises(ValueError, match="per_sample_weights must be"):
        tn.tt_embedding_bag(ttm, rows, None, w)                      # [12] against rows [2, 6]
    with pytest.raises(ValueError, match="mode 'sum' only"):
        tn.tt_embedding_bag(ttm, flat, off, w, "mean")


@pytest.mark.parametrize("form", [None] + ec.BAG_FORMS, ids=["embedding"] + [f[0] for f in ec.BAG_FORMS])
@pytest.mark.parametrize("name", NAMES)
def test_gradients_of_the_cores_on_the_host(name, form):
    """fp64 on the CPU against autograd through the dense matrix.  Both sides sum the same few hundred products of O(1) numbers
    in fp64 in another order: 1e-10 of the largest gradient entry is six orders above that rounding and far below any wrong term
    (``test_lookup_host.py`` reasons the same way).  The weights get their gradient from autograd too."""
    tt, idims, odims, nrows, ncols = ec.case(name, torch.float64)
    if form is None:
        rows, offsets, w, mode, seg = lc.lookup_rows(nrows), None, None, "sum", None
        g = ec.cotangent((2, 6, ncols))
    else:
        rows, offsets, w, mode, seg = ec.bag_operands(form, nrows, torch.float64)
        g = ec.cotangent((len(seg) - 1, ncols))
    _, theirs = ec.reference(tt, rows, seg, w, mode, g)
    ours = [c.clone().requires_grad_(True) for c in tt]
    ttm = tn.TTMatrix(ours, None, idims, odims)
    wl = None if w is None else w.clone().requires_grad_(True)
    y = tn.tt_embedding(ttm, rows) if form is None else tn.tt_embedding_bag(ttm, rows, offsets, wl, mode)
    assert y.requires_grad
    (y * g).sum().backward()
    for a, b in zip(ours, theirs):
        assert a.grad is not None and float((a.grad - b).abs().max()) <= 1e-10 * float(b.abs().max())
    if wl is not None:
        rowsum = (ec.dense([c.double() for c in tt])[rows.reshape(-1)] * g[torch.searchsorted(torch.tensor(seg[1:]), torch.arange(12),
                                                                                                  right=True)]).sum(dim=1)
        assert float((wl.grad.reshape(-1) - rowsum).abs().max()) <= 1e-10 * float(rowsum.abs().max())


def test_host_mirrors_against_autograd():
    """The three ``_hostops`` mirrors in fp64 against autograd through the forward contract (the same products in another order:
    1e-12 of the largest entry)."""
    P, D, R, I, O, S = 9, 3, 4, 7, 2, 3
    X, G, idx, dY = ec.grad_operands((P, D, R, I, O, S), torch.float64, rows_x=7)
    xrow = torch.randint(0, 7, (P,), generator=torch.Generator().manual_seed(1))
    Xl, Gl = X.clone().requires_grad_(True), G.clone().requires_grad_(True)
    Zl = X[xrow].clone().requires_grad_(True)
    v = ec.wrapped(idx, I)
    assert bool((idx < 0).any()) and int(torch.bincount(v, minlength=I).min()) == 0   # negatives wrap; a slice nobody asks for
    torch.einsum("pdr,rpos->pdos", Xl[xrow], Gl[:, v]).backward(dY)
    torch.einsum("pdr,rpos->pdos", Zl, G[:, v]).backward(dY)
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())
    dG = _hostops.ttm_lookup_grad_core(X, xrow, dY, idx, I)
    assert tuple(dG.shape) == (R, I, O, S) and close(dG, Gl.grad)
    assert bool((dG[:, torch.bincount(v, minlength=I) == 0] == 0).all())
    assert close(_hostops.ttm_lookup_grad_core(X[xrow], None, dY, idx, I), Gl.grad)
    dX = _hostops.ttm_lookup_grad_input(dY, G, idx)
    assert tuple(dX.shape) == (P, D, R) and close(dX, Zl.grad)
    for C in (1, 15):
        Y, w, perm, seg = ec.segment_operands(C, torch.float64)
        for ww, pp in ((None, None), (w, None), (None, perm), (w, perm)):
            out64, _ = ec.segment_truth_and_bound(Y, seg, ww, pp, torch.float64)
            out = _hostops.segment_sum(Y, seg, ww, pp)
            assert tuple(out.shape) == (len(ec.SEG_LENGTHS), C) and close(out, out64)
            assert bool((out[0] == 0).all()) and bool((out[-1] == 0).all())
    Yl, wl = Y.clone().requires_grad_(True), w.clone().requires_grad_(True)
    gs = ec.cotangent((len(ec.SEG_LENGTHS), C))
    _hostops.segment_sum(Yl, seg, wl).backward(gs)
    bag = torch.repeat_interleave(torch.arange(len(ec.SEG_LENGTHS)), torch.tensor(ec.SEG_LENGTHS))
    assert close(Yl.grad, gs[bag] * w[:, None]) and close(wl.grad, (gs[bag] * Y).sum(dim=1))


def test_wiring():
    assert tn.tt_embedding is tn.embedding.tt_embedding and tn.tt_embedding_bag is tn.embedding.tt_embedding_bag
    assert tn.embedding.__all__ == ["tt_embedding", "tt_embedding_bag"]
    assert tn.lookup.__all__ == ["tt_lookup"]
    assert callable(tn.autodiff.tt_rows) and "tt_rows" not in tn.autodiff.__all__
    with open(os.path.join(mc.ROOT, "include", "ttround_hip.h")) as f:
        header = f.read()
    define = header.index("#define TTR_ABI_VERSION")
    for name in ("ttr_ttm_lookup_grad_core_slab_rows", "ttr_ttm_lookup_grad_core_workspace_bytes", "ttr_ttm_lookup_grad_core",
                 "ttr_ttm_lookup_grad_input_workspace_bytes", "ttr_ttm_lookup_grad_input", "ttr_segment_sum"):
        assert re.search(r"\b{}\b".format(name), header[:define]), "{} is not named in the comment above TTR_ABI_VERSION".format(name)
        assert re.search(r"\bint(64_t)?\s+{}\s*\(".format(name), header[define:]), name
        assert name in _hip.EXPORTED_SYMBOLS
    assert _hip.ABI_VERSION == 17
    with open(os.path.join(mc.ROOT, "tntorch_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^\s+ttr_ttlookup_grad\.hip\b", f.read(), re.M)
    for mod in (_hipops, _hostops):
        assert callable(mod.ttm_lookup_grad_core) and callable(mod.ttm_lookup_grad_input) and callable(mod.segment_sum)
    assert callable(_hipops.tt_lookup_steps)
    with open(os.path.join(mc.ROOT, "DESIGN.md")) as f:
        assert re.search(r"^#+\s*31\b", f.read(), re.M)


def test_slab_rule_reads_its_arguments_only():
    """The slab query is host arithmetic (no device here): the floor of 256 rows, a multiple of 32, about 1024 workgroups."""
    rows = _hip.ttm_lookup_grad_core_slab_rows
    assert rows(torch.float32, 65, 65, 33, 5, 5, 16) == 256 and rows(torch.float64, 300, 17, 3, 5, 1, 1) == 256
    big = rows(torch.float32, 1 << 20, 32, 16, 100, 4, 1)
    assert big == (1 << 25) // 1024 and big % 32 == 0
    assert rows(torch.float32, 1 << 20, 32, 16, 100, 64, 64) == -(-(1 << 25) // (1024 // 64))
    assert _hip.ttm_lookup_grad_core_workspace_bytes(torch.float32, 0, 1, 1, 1, 1, 1) > 0
    with pytest.raises(ValueError):
        rows(torch.float32, 5, 0, 1, 1, 1, 1)

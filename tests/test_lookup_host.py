"""``tn.tt_lookup`` on the CPU (the host mirror, plain torch): values within the derived chain bound, the shapes and dtypes of
``rows``, the refusals, the gradients of the cores against autograd through the dense matrix, and the wiring of the feature
(exports, the two C entries in the header, the build recipe, the design section)."""
import os
import re

import numpy as np
import pytest
import torch

import lookup_cases as lc
import matrix_cases as mc
import tntorch_amd as tn
from tntorch_amd import _hip, _hipops, _hostops

DTYPES = [torch.float32, torch.float64]
NAMES = ["ref", "three", "single"]


def _matrix(name, dt):
    idims, odims = mc.RANDOM_CASES[name][:2]
    tt, _, _ = mc.random_cores(name, dt)
    return tn.TTMatrix(tt, None, idims, odims), tt, int(np.prod(idims)), int(np.prod(odims))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_rows_on_the_host(name, dt):
    ttm, tt, nrows, ncols = _matrix(name, dt)
    kept = [c.clone() for c in tt]
    rows = lc.lookup_rows(nrows)
    y64, bound = lc.truth_and_bound(tt, rows, dt)
    y = tn.tt_lookup(ttm, rows)
    assert y.device.type == "cpu" and y.dtype == dt and tuple(y.shape) == (2, 6, ncols)
    mc.assert_within(y, y64, bound, "tt_lookup {} {}".format(name, dt))
    flat = rows.reshape(-1)
    for r in (flat, flat.int(), flat.tolist(), tuple(flat.tolist()), flat.numpy()):
        y1 = tn.tt_lookup(ttm, r)
        assert y1.dtype == dt and tuple(y1.shape) == (12, ncols)
        mc.assert_within(y1, y64.reshape(12, ncols), bound.reshape(12, ncols), "1-D rows")
    assert all(torch.equal(a, b) for a, b in zip(ttm.cores, kept))


def test_noncontiguous_cores_and_empty_rows_on_the_host():
    dt = torch.float64
    ttm, tt, nrows, ncols = _matrix("three", dt)
    rows = lc.lookup_rows(nrows)
    y64, bound = lc.truth_and_bound(tt, rows, dt)
    cores = [torch.cat([c, c], dim=2)[:, :, :c.shape[2], :] for c in tt]
    mc.assert_within(tn.tt_lookup(tn.TTMatrix(cores, None, [4, 3, 5], [2, 6, 3]), rows), y64, bound, "strided cores")
    for empty in (torch.zeros((0,), dtype=torch.int64), torch.zeros((3, 0), dtype=torch.int32), []):
        y = tn.tt_lookup(ttm, empty)
        assert y.dtype == dt and tuple(y.shape) == tuple(torch.as_tensor(empty).shape) + (ncols,)


def test_refusals_on_the_host():
    ttm, tt, nrows, _ = _matrix("three", torch.float64)
    rows = lc.lookup_rows(nrows)
    with pytest.raises(ValueError, match="must be a TTMatrix"):
        tn.tt_lookup(tt, rows)
    with pytest.raises(ValueError, match="batched"):
        tn.tt_lookup(tn.TTMatrix([c[None] for c in tt], None, [4, 3, 5], [2, 6, 3]), rows)
    with pytest.raises(ValueError, match="boundary ranks"):
        tn.tt_lookup(tn.TTMatrix(tt[1:], None, [3, 5], [6, 3]), rows)
    with pytest.raises(ValueError, match="float32 or float64"):
        tn.tt_lookup(tn.TTMatrix([c.half() for c in tt], None, [4, 3, 5], [2, 6, 3]), rows)
    with pytest.raises(ValueError, match="same dtype"):
        tn.tt_lookup(tn.TTMatrix([tt[0], tt[1].float(), tt[2]], None, [4, 3, 5], [2, 6, 3]), rows)
    with pytest.raises(ValueError, match="same device"):
        tn.tt_lookup(ttm, rows.to("meta"))
    for bad in (rows.double(), rows > 0, [0.5, 1.0]):
        with pytest.raises(ValueError, match="int32 or int64"):
            tn.tt_lookup(ttm, bad)
    for name in NAMES:
        m, _, n, _ = _matrix(name, torch.float32)
        for bad in (n, -n - 1):
            with pytest.raises(IndexError, match="outside the matrix"):
                tn.tt_lookup(m, torch.tensor([0, bad, 1]))
        assert tuple(tn.tt_lookup(m, [n - 1, -n]).shape)[0] == 2


@pytest.mark.parametrize("name", NAMES)
def test_gradients_of_the_cores_on_the_host(name):
    """fp64 on the CPU against autograd through the dense matrix (a plain contraction and a gather).  Both sides sum the same
    few hundred products of O(1) numbers in fp64 in another order: 1e-10 of the largest gradient entry is six orders above
    that rounding and far below any wrong term (tests/test_autodiff_gpu.py reasons the same way)."""
    idims, odims = mc.RANDOM_CASES[name][:2]
    tt, _, _ = mc.random_cores(name, torch.float64)
    nrows, ncols = int(np.prod(idims)), int(np.prod(odims))
    rows = lc.lookup_rows(nrows)
    w = torch.randn((2, 6, ncols), dtype=torch.float64, generator=torch.Generator().manual_seed(8))

    def dense(cores):
        acc = None
        for G in cores:
            acc = G if acc is None else torch.einsum("aiob,bjpc->aijopc", acc, G).reshape(acc.shape[0], acc.shape[1] * G.shape[1],
                                                                                           acc.shape[2] * G.shape[2], G.shape[3])
        return acc[0, :, :, 0]

    ours = [c.clone().requires_grad_(True) for c in tt]
    y = tn.tt_lookup(tn.TTMatrix(ours, None, idims, odims), rows)
    assert y.requires_grad
    (y * w).sum().backward()
    theirs = [c.clone().requires_grad_(True) for c in tt]
    (dense(theirs)[rows] * w).sum().backward()
    for a, b in zip(ours, theirs):
        assert a.grad is not None and float((a.grad - b.grad).abs().max()) <= 1e-10 * float(b.grad.abs().max())


def test_wiring():
    assert tn.tt_lookup is tn.lookup.tt_lookup
    assert tn.lookup.__all__ == ["tt_lookup"]
    assert tn.matrix.__all__ == ["TTMatrix", "CPMatrix", "tt_multiply", "cp_multiply"]
    with open(os.path.join(mc.ROOT, "include", "ttround_hip.h")) as f:
        header = f.read()
    define = header.index("#define TTR_ABI_VERSION")
    for name in ("ttr_ttm_lookup_workspace_bytes", "ttr_ttm_lookup_step"):
        assert name in header[:define], "{} is not named in the comment above TTR_ABI_VERSION".format(name)
        assert re.search(r"\bint(64_t)?\s+{}\s*\(".format(name), header[define:]), name
        assert name in _hip.EXPORTED_SYMBOLS
    assert _hip.ABI_VERSION == 17
    with open(os.path.join(mc.ROOT, "tntorch_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^\s+ttr_ttlookup\.hip\b", f.read(), re.M)
    for mod in (_hipops, _hostops):
        assert callable(mod.tt_lookup_chain)
    assert callable(_hip.ttm_lookup_step)
    with open(os.path.join(mc.ROOT, "DESIGN.md")) as f:
        assert re.search(r"^#+\s*27\b", f.read(), re.M)

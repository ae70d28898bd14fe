"""``tn.tt_lookup`` on a real MI355X: the rows of ``matrix_cases``' random TT-matrices against the dense fp64 truth within the
derived chain bound; the shapes and dtypes of ``rows``; that a row's bits do not depend on the batch; that the device path is
exactly ``d - 1`` launches of ttr_ttm_lookup_step; and every refusal."""
import numpy as np
import pytest
import torch

import lookup_cases as lc
import matrix_cases as mc
import tntorch_amd as tn
from tntorch_amd import _hip

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
NAMES = ["ref", "three", "single"]


def _matrix(name, dt):
    idims, odims = mc.RANDOM_CASES[name][:2]
    tt, _, _ = mc.random_cores(name, dt)
    return tn.TTMatrix([c.cuda() for c in tt], None, idims, odims), tt, int(np.prod(idims)), int(np.prod(odims))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_rows_on_the_device(name, dt):
    ttm, tt, nrows, ncols = _matrix(name, dt)
    rows = lc.lookup_rows(nrows)                                            # [2, 6]: duplicates, negatives, both ends
    y64, bound = lc.truth_and_bound(tt, rows, dt)
    y = tn.tt_lookup(ttm, rows.cuda())
    assert y.is_cuda and y.device == ttm.cores[0].device and y.dtype == dt and tuple(y.shape) == (2, 6, ncols)
    mc.assert_within(y, y64, bound, "tt_lookup {} {}".format(name, dt))
    flat = rows.reshape(-1)
    for r in (flat.cuda(), flat.int().cuda(), flat.tolist(), tuple(flat.tolist()), flat.numpy()):   # 1-D: int64, int32, list, tuple, numpy
        y1 = tn.tt_lookup(ttm, r)
        assert y1.is_cuda and y1.dtype == dt and tuple(y1.shape) == (12, ncols)
        assert torch.equal(y1, y.reshape(12, ncols))
    for k in (0, 5, 11):                                                    # a row's bits do not depend on the batch
        assert torch.equal(tn.tt_lookup(ttm, flat[k:k + 1].cuda())[0], y.reshape(12, ncols)[k])
    assert all(torch.equal(a.cpu(), b) for a, b in zip(ttm.cores, tt))      # the cores are not modified


@pytest.mark.parametrize("dt", DTYPES)
def test_noncontiguous_cores_and_empty_rows(dt):
    ttm, tt, nrows, ncols = _matrix("three", dt)
    rows = lc.lookup_rows(nrows)
    y64, bound = lc.truth_and_bound(tt, rows, dt)
    cores = [torch.cat([c, c], dim=2)[:, :, :c.shape[2], :] for c in ttm.cores]
    assert not any(c.is_contiguous() for c in cores)
    mc.assert_within(tn.tt_lookup(tn.TTMatrix(cores, None, [4, 3, 5], [2, 6, 3]), rows.cuda()), y64, bound, "strided cores")
    for empty in (torch.zeros((0,), dtype=torch.int64).cuda(), torch.zeros((3, 0), dtype=torch.int32).cuda(), []):
        y = tn.tt_lookup(ttm, empty)
        assert y.is_cuda and y.dtype == dt and tuple(y.shape) == tuple(torch.as_tensor(empty).shape) + (ncols,)


def test_launch_counts(monkeypatch):
    """d >= 2: d - 1 launches of ttr_ttm_lookup_step and nothing else from the library; d = 1: no library call."""
    calls = []
    real = _hip._call

    def counting(name, *args):
        calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(_hip, "_call", counting)
    for name, want in (("three", ["ttr_ttm_lookup_step"] * 2), ("ref", ["ttr_ttm_lookup_step"]), ("single", [])):
        ttm, _, nrows, _ = _matrix(name, torch.float32)
        del calls[:]
        tn.tt_lookup(ttm, lc.lookup_rows(nrows).cuda())
        assert calls == want, name


def test_refusals_on_the_device():
    ttm, tt, nrows, _ = _matrix("three", torch.float64)
    rows = lc.lookup_rows(nrows).cuda()
    with pytest.raises(ValueError, match="must be a TTMatrix"):
        tn.tt_lookup(ttm.cores, rows)
    with pytest.raises(ValueError, match="batched"):
        tn.tt_lookup(tn.TTMatrix([c[None] for c in ttm.cores], None, [4, 3, 5], [2, 6, 3]), rows)
    with pytest.raises(ValueError, match="boundary ranks"):
        tn.tt_lookup(tn.TTMatrix(ttm.cores[1:], None, [3, 5], [6, 3]), rows)
    with pytest.raises(ValueError, match="float32 or float64"):
        tn.tt_lookup(tn.TTMatrix([c.half() for c in ttm.cores], None, [4, 3, 5], [2, 6, 3]), rows)
    with pytest.raises(ValueError, match="same dtype"):
        tn.tt_lookup(tn.TTMatrix([ttm.cores[0], ttm.cores[1].float(), ttm.cores[2]], None, [4, 3, 5], [2, 6, 3]), rows)
    with pytest.raises(ValueError, match="same device"):
        tn.tt_lookup(tn.TTMatrix([ttm.cores[0], ttm.cores[1].cpu(), ttm.cores[2]], None, [4, 3, 5], [2, 6, 3]), rows)
    with pytest.raises(ValueError, match="same device"):
        tn.tt_lookup(ttm, rows.cpu())
    for bad in (rows.double(), rows > 0, [0.5, 1.0]):
        with pytest.raises(ValueError, match="int32 or int64"):
            tn.tt_lookup(ttm, bad)
    for name in NAMES:                                                      # d = 3, 2 and 1
        m, _, n, _ = _matrix(name, torch.float32)
        for bad in (n, -n - 1):
            with pytest.raises(IndexError, match="outside the matrix"):
                tn.tt_lookup(m, torch.tensor([0, bad, 1]).cuda())
        assert tuple(tn.tt_lookup(m, [n - 1, -n]).shape)[0] == 2


def test_grad_mode_is_refused_not_cut():
    ttm, _, nrows, ncols = _matrix("three", torch.float64)
    rows = lc.lookup_rows(nrows).cuda()
    want = tn.tt_lookup(ttm, rows)
    for k in range(3):
        cores = [c.clone() for c in ttm.cores]
        cores[k].requires_grad_(True)
        m = tn.TTMatrix(cores, None, [4, 3, 5], [2, 6, 3])
        with pytest.raises(NotImplementedError, match="tt_lookup is not differentiable on the device"):
            tn.tt_lookup(m, rows)
        with torch.no_grad():
            y = tn.tt_lookup(m, rows)
        assert not y.requires_grad and torch.equal(y, want)

"""tn.minimum / tn.argmin / tn.maximum / tn.argmax on device tensors (MI355X): the cases of tests/minimize_cases.py in fp64 and
fp32, where the results live, and how often the call reads from the device.

fp64: the position is an optimiser of the case's dense tensor, exactly (``dense[argmin] == dense.min()``), and the value is the
train's entry there.  The value is a fibre sample (two ttr_gemm: left interface x core x right interface), ``t[pos]`` a chain of
gather steps from the left and ``t.torch()`` a third order of the same products, so the three agree bit for bit where the
products are exact (quad8, quad5764: the identity-padded train multiplies the entries by 0 and 1 only; there all of the issue's
equalities are asserted on the device train) and within ``minimize_cases.value_bound`` on sinquad and randn3, whose cores are
dense.  On sinquad the optimisers are exactly tied in the dense tensor and its rank-4 train carries rounding noise (measured on
the device: t.torch() at the found minimiser -2.0612481317439855 against its own minimum -2.0612481317439877), so the position is
judged on the dense tensor the train was built from, not on ``t.torch()``.
fp32: |minimum - dense.min()| and dense[argmin] - dense.min() within minimize_cases.FP32_RTOL of max |dense|."""
import pytest
import torch

import minimize_cases as mc
import tntorch_amd as tn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_BUILT = {}


def case(name, dtype):
    """(device train, its t.torch() on the device, the dense fp64 tensor of the case on the CPU)"""
    if (name, dtype) not in _BUILT:
        t, d = mc.build(name, tn)
        td = mc.to(t, tn, dtype, DEV)
        _BUILT[(name, dtype)] = (td, td.torch(), d)
    return _BUILT[(name, dtype)]


def call(fn, t, s):
    mc.seed(s)
    return getattr(tn, fn)(t)


@pytest.mark.parametrize("fn", mc.FUNCTIONS)
@pytest.mark.parametrize("s", mc.SEEDS)
@pytest.mark.parametrize("name", mc.CASES)
def test_fp64(name, s, fn):
    t, td, d = case(name, torch.float64)
    best = d.min() if fn in ("minimum", "argmin") else d.max()
    pos = call("argmin" if fn in ("minimum", "argmin") else "argmax", t, s)
    assert isinstance(pos, tuple) and len(pos) == t.dim() and all(type(x) is int for x in pos)
    assert float(d[pos]) == float(best)                        # an optimiser of the dense tensor
    if name in mc.UNIQUE:
        assert pos == tuple(int(x) for x in torch.nonzero(d == best)[0])
    if fn.startswith("arg"):
        return
    v = call(fn, t, s)
    assert isinstance(v, torch.Tensor) and v.dim() == 0 and v.dtype == torch.float64 and v.device == torch.device(DEV)
    at = t[pos]
    at = at.torch() if hasattr(at, "torch") else at
    tbest = td.min() if fn == "minimum" else td.max()
    if name in mc.EXACT_TRAIN:
        assert float(v) == float(at) == float(td[pos]) == float(tbest) == float(best)   # the sample itself
    else:
        bound = mc.value_bound(t, pos)
        train_err = float((td.cpu() - d).abs().max())           # the train against the dense tensor it was built from
        print("fp64 {} s{} {}: value {!r}, t[pos] {!r}, t.torch() optimum {!r}, dense optimum {!r}, bound {:.2e} + {:.2e}".format(
            name, s, fn, float(v), float(at), float(tbest), float(best), bound, train_err))
        assert abs(float(v) - float(at)) <= bound and abs(float(v) - float(tbest)) <= bound + 2 * train_err
        assert abs(float(v) - float(best)) <= bound + train_err


@pytest.mark.parametrize("fn", mc.FUNCTIONS)
@pytest.mark.parametrize("s", mc.SEEDS)
@pytest.mark.parametrize("name", mc.CASES)
def test_fp32(name, s, fn):
    t, d, _ = case(name, torch.float32)
    lo = fn in ("minimum", "argmin")
    best = float(d.min() if lo else d.max())
    scale = float(d.abs().max())
    r = call(fn, t, s)
    if fn.startswith("arg"):
        assert isinstance(r, tuple) and len(r) == t.dim() and all(type(x) is int for x in r)
        dev = (float(d[r]) - best) * (1 if lo else -1)
        assert dev >= 0
    else:
        assert isinstance(r, torch.Tensor) and r.dim() == 0 and r.dtype == torch.float32 and r.device == torch.device(DEV)
        dev = abs(float(r) - best)
    print("fp32 {} s{} {}: deviation {:.3e} of max |dense| (measured bound {:.1e})".format(name, s, fn, dev / scale, mc.FP32_MEASURED))
    assert dev <= mc.FP32_RTOL * scale


def test_reads_from_the_device(monkeypatch):
    """One readback per sweep (validation error, invalid flag and best value in one stacked copy) and one after the last sweep
    (the position); ``return_info`` then copies the index sets, as ``cross`` always does.  Counted on the copies a device tensor
    can make to the host from Python: .cpu(), .item(), .tolist(), .numpy() and the conversions that go through .item()."""
    t = case("quad5764", torch.float64)[0]
    counts = {}

    def counted(name):
        orig = getattr(torch.Tensor, name)

        def wrapper(self, *a, **k):
            if self.is_cuda:
                counts[name] = counts.get(name, 0) + 1
            return orig(self, *a, **k)

        monkeypatch.setattr(torch.Tensor, name, wrapper)

    for name in ("cpu", "item", "tolist", "numpy", "__bool__", "__int__", "__float__", "__index__"):
        counted(name)
    mc.seed(0)
    _, info = tn.cross(tensors=t, rmax=10, max_iter=3, verbose=False, return_info=True, _minimize=True)
    monkeypatch.undo()
    sweeps, N = len(info["val_epss"]), t.dim()
    assert sweeps == 3
    sets_copied = 2 * N + len(info["left_locals"])             # lsets, rsets, left_locals: return_info's copies
    assert counts == {"cpu": sweeps + sets_copied, "tolist": 1}, counts
    assert info["min"].device == torch.device(DEV) and info["argmin"] == call("argmin", t, 0)


def test_refusals():
    t = case("quad8", torch.float64)[0]
    with pytest.raises(ValueError, match="Batched"):
        tn.minimum(tn.rand([4] * 3, ranks_tt=2, batch=True))
    with pytest.raises(ValueError, match="Invalid return value"):
        tn.minimum(t, function=lambda x: torch.where(x > 3, x * float("nan"), x))
    with pytest.raises(NotImplementedError, match="CP"):
        tn.minimum(tn.Tensor([torch.rand(6, 2, dtype=torch.float64, device=DEV) for _ in range(3)]))
    big = tn.Tensor([torch.rand(1, 200, 200, device=DEV), torch.rand(200, 200, 200, device=DEV), torch.rand(200, 200, 1, device=DEV)])
    with pytest.raises(NotImplementedError, match="ranks above"):
        tn.minimum(big, rmax=200, ranks_tt=200)

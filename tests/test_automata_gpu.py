"""The Boolean layer on the MI355X through the public API: ``tn.accepted_inputs`` on device masks equals the CPU mirror's result row
for row, stays on the device and reads the host a bounded number of times; ``tn.mask``, ``tn.only`` and ``tn.partialset`` on the
device equal the CPU path.  Integer-exact: no tolerances."""
import pytest
import torch

import automata_cases as ac
import tntorch_amd as tn

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64


def to_dev(t, dtype=None):
    return tn.Tensor([c.to(DEV, dtype or c.dtype) for c in t.cores], Us=[None if U is None else U.to(DEV, dtype or U.dtype) for U in t.Us])


def to_cpu(t):
    return tn.Tensor([c.cpu() for c in t.cores], Us=[None if U is None else U.cpu() for U in t.Us])


def check_accepted(t_cpu, dtype=None):
    ref = tn.accepted_inputs(t_cpu)
    X = tn.accepted_inputs(to_dev(t_cpu, dtype))
    assert X.is_cuda and X.dtype == torch.int64 and X.shape == ref.shape
    assert torch.equal(X.cpu(), ref)
    return ref


@pytest.mark.parametrize("dtype", [torch.float32, F64])
def test_weight_mask_16_8(dtype):
    ref = check_accepted(tn.weight_mask(16, 8), dtype)
    assert ref.shape == (12870, 16) and bool((ref.sum(dim=1) == 8).all())


def test_weight_mask_with_mixed_alphabets():
    ref = check_accepted(tn.weight_mask(10, [2, 5], nsymbols=[2, 3] * 5))
    assert bool(((ref.sum(dim=1) == 2) | (ref.sum(dim=1) == 5)).all())


def test_weight_multiplicities():
    ref = check_accepted(tn.weight(6))
    assert ref.shape == (6 * 32, 6)   # every string as often as its weight: sum of weights = N 2^(N-1)


def test_constructors_on_the_device():
    m = tn.weight_mask(6, 3, dtype=F64, device=DEV)
    assert all(c.is_cuda and c.dtype == F64 for c in m.cores)
    assert torch.equal(tn.accepted_inputs(m).cpu(), ac.combinations_matrix(6, 3))
    assert tn.accepted_inputs(tn.false(3, device=DEV)).shape == (0, 3)
    with pytest.raises(ValueError):
        tn.accepted_inputs(m * 0.5)


def test_mask_that_went_through_round_tt():
    """x | y | z on 8 symbols, built with ranks 8 and rounded: the cores are not integers any more, the counts still round
    consistently."""
    s = tn.symbols(8, dtype=F64)
    m = (s[0] | s[3] | s[6]) & tn.weight_mask(8, [2, 3, 4], dtype=F64)
    truth = tn.accepted_inputs(m)
    m.round_tt(eps=1e-12)
    assert any(bool((c != c.round()).any()) for c in m.cores)
    ref = check_accepted(m)
    assert torch.equal(ref, truth)


def test_host_reads_are_bounded(monkeypatch):
    """The number of rows, one frontier size per mode and the consistency word: at most N + 2 reads, whatever the size."""
    def count(t):
        torch.cuda.synchronize()
        n = [0]
        for cls, name in ((torch.Tensor, "item"), (torch.Tensor, "tolist"), (torch.Tensor, "cpu"), (torch.cuda, "synchronize")):
            orig = getattr(cls, name)

            def wrap(*a, _o=orig, **k):
                n[0] += 1
                return _o(*a, **k)

            monkeypatch.setattr(cls, name, wrap)
        X = tn.accepted_inputs(t)
        monkeypatch.undo()
        assert X.is_cuda
        return n[0]

    small, large = tn.weight_mask(12, 2, device=DEV), tn.weight_mask(12, 6, device=DEV)
    assert count(small) <= 12 + 2 and count(large) <= 12 + 2 and count(small) == count(large)


def test_mask_only_and_partialset_equal_the_cpu_path():
    z = ac.fixture()
    t = tn.Tensor(ac.golden_cores("mask_t"))
    idxs = [torch.from_numpy(z["mask_idx{}".format(n)]) for n in range(3)]
    t.idxs = idxs
    m = tn.Tensor(ac.golden_cores("mask_m"))
    td = to_dev(t)
    td.idxs = [i.to(DEV) for i in idxs]
    out = tn.mask(td, to_dev(m))
    assert all(c.is_cuda for c in out.cores) and torch.equal(out.torch().cpu(), tn.mask(t, m).torch())
    assert torch.equal(tn.mask(td, m).torch().cpu(), tn.mask(t, m).torch())   # a CPU mask is moved to t's device

    x, y, w, v = tn.symbols(4, dtype=F64)
    f = (x & ~w) | (x & w)
    fd = to_dev(f)
    assert tn.relevant_symbols(fd) == tn.relevant_symbols(f) == [0]
    od = tn.only(fd)
    assert all(c.is_cuda for c in od.cores) and torch.equal(od.torch().cpu(), tn.only(f).torch())

    p = tn.Tensor(ac.golden_cores("pset_t"))
    for order, mask in ((1, None), ([1, 2], tn.symbols(3, dtype=F64)[0])):
        ref = tn.partialset(p, order, mask=mask, bounds=z["pset_bounds"].tolist())
        got = tn.partialset(to_dev(p), order, mask=None if mask is None else to_dev(mask), bounds=z["pset_bounds"].tolist())
        assert all(c.is_cuda for c in got.cores) and torch.equal(got.torch().cpu(), ref.torch())
        assert all(torch.equal(a.cpu(), b) for a, b in zip(got.idxs, ref.idxs))

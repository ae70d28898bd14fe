"""``tn.sample`` on device tensors (MI355X): the cases of tests/sample_cases.py in fp64 and fp32 against the reference's samples,
the host mirror on the same thresholds, the exact cases, a long fp32 train, the refusals and the number of readbacks."""
import pytest
import torch

import sample_cases as sc
import tntorch_amd as tn
from tntorch_amd import _hip, tools

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.float64]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(sc.CASES))
def test_golden_cases(name, dtype):
    cs = sc.cores(name, dtype)
    t = tn.Tensor([c.to(DEV) for c in cs])
    X = tn.sample(t, sc.P_GOLDEN, seed=sc.SEED_GOLDEN)
    assert X.dtype == torch.int64 and X.device == torch.device(DEV) and tuple(X.shape) == (sc.P_GOLDEN, len(cs))
    U = sc.thresholds(sc.P_GOLDEN, len(cs))
    print("{} {}: {} rows differ from the reference".format(name, dtype, sc.explained(X, sc.golden(name), cs, U, dtype)))
    assert bool(sc.valid(cs, X, U, dtype).all())
    # the host mirror on the same thresholds
    Xh = tools._sample_from_thresholds(tn.Tensor(cs), U)
    print("{} {}: {} rows differ from the host mirror".format(name, dtype, sc.explained(X, Xh, cs, U, dtype)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_weight_mask_members(dtype):
    cs = [c.to(dtype) for c in tn.weight_mask(6, 2).cores]
    X = tn.sample(tn.Tensor([c.to(DEV) for c in cs]), 2000, seed=1)
    assert bool((X.sum(dim=1) == 2).all()) and X.min() >= 0 and X.max() <= 1
    assert torch.equal(X.cpu(), tn.sample(tn.Tensor(cs), 2000, seed=1))   # small integers: exact on either side


def test_seed_none_draws_on_the_device():
    t = tn.Tensor(sc.cores("pos", torch.float64, DEV))
    torch.manual_seed(3)
    X = tn.sample(t, 257)
    torch.manual_seed(3)
    U = torch.rand((257, 4), dtype=torch.float64, device=DEV)
    assert torch.equal(X, tools._sample_from_thresholds(t, U))
    torch.manual_seed(3)
    assert torch.equal(X, tn.sample(t, 257))
    assert tuple(tn.sample(t, 0).shape) == (0, 4)


def test_long_fp32_train():
    """40 modes of entries near 1e-2: unscaled fp32 left vectors and right vectors would underflow on the way."""
    g = torch.Generator().manual_seed(8)
    N, I, r = 40, 4, 3
    ranks = [1] + [r] * (N - 1) + [1]
    cs = [(1e-2 * (0.5 + torch.rand((ranks[n], I, ranks[n + 1]), generator=g, dtype=torch.float64))).float() for n in range(N)]
    U = torch.rand((500, N), generator=g, dtype=torch.float64)
    X = tools._sample_from_thresholds(tn.Tensor([c.to(DEV) for c in cs]), U.to(DEV))
    assert bool(sc.valid(cs, X, U, torch.float32).all())


def test_refusals():
    big = _hip.sample_max_rank() + 1
    t = tn.Tensor([torch.ones((1, 2, big), device=DEV), torch.ones((big, 2, 1), device=DEV)])
    with pytest.raises(ValueError, match="rank"):
        tn.sample(t, 4, seed=0)
    with pytest.raises(ValueError):
        tn.sample(tn.Tensor([torch.zeros((1, 3, 2), device=DEV), torch.zeros((2, 3, 1), device=DEV)]), 4, seed=0)


def test_one_readback_per_call(monkeypatch):
    """Counted on the copies a device tensor can make to the host from Python, as tests/test_minimize_gpu.py counts them."""
    t = tn.Tensor(sc.cores("pos", torch.float32, DEV))
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
    tn.sample(t, 1000, seed=0)
    tn.sample(t, 1000)
    monkeypatch.undo()
    assert counts == {"item": 2}, counts

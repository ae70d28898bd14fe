"""``tntorch_amd/anova.py`` on device tensors (a real MI355X): the golden cases of tests/golden/anova_f64.npz in both dtypes, the
device against the host mirror at ranks and mode sizes that are no tile multiples, the route above the fused kernel's rank
limit, and a train whose mean dominates its variance (fp32)."""
import pytest
import torch

import anova_cases as ac
import pce_cases as pc
import tntorch_amd as tn
from tntorch_amd import _hip

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]


def _on_device(r, dt):
    x = r.cores[0] if hasattr(r, "cores") else r
    assert x.is_cuda and x.dtype == dt


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("q", sorted(ac.CASES))
def test_golden_on_the_device(q, dt):
    """fp64: 1e-10 of the brute-force truth; fp32: 1e-4 absolute (the CPU mirror's fp32 run is off by 1e-7)."""
    r = ac.CASES[q](tn, dt, "cuda")
    _on_device(r, dt)
    err = ac.abs_err(r, q)
    print(q, dt, "abs. error", err)
    assert err < (1e-4 if dt == torch.float32 else 1e-10), (q, err)


def _random_train(shape, ranks, dt, seed):
    g = torch.Generator().manual_seed(seed)
    rs = [1] + list(ranks) + [1]
    cores = [torch.rand(rs[n], s, rs[n + 1], generator=g, dtype=torch.float64) / rs[n] for n, s in enumerate(shape)]
    marg = [torch.rand(s, generator=g, dtype=torch.float64) + 0.1 for s in shape]
    return [c.to(dt) for c in cores], [m.to(dt) for m in marg]


def _masks(N, dt, dev):
    x = tn.symbols(N, dtype=dt, device=dev)
    return {"only_x0": tn.only(x[0]), "x1_not_x2": x[1] & ~x[2], "weight": tn.weight(N, dtype=dt, device=dev),
            "one_hot": tn.weight_one_hot(N, dtype=dt, device=dev)}


@pytest.fixture(scope="module")
def mirror():
    """The host mirror's fp64 results on the two random trains, computed once: ranks 17 with I = 33 (no tile multiples, five
    chunks of i), and ranks max_rank + 1 with I = 2 (above the fused kernel's limit)."""
    out = {}
    for name, shape, ranks in (("r17", [33, 33, 33], [17, 17]), ("above", [2, 2, 2], [_hip.mode_sandwich_max_rank() + 1] * 2)):
        cores, marg = _random_train(shape, ranks, torch.float64, 7)
        t = tn.Tensor(cores)
        out[name] = {k: ac.value(tn.sobol(t, m, marg)) for k, m in _masks(3, torch.float64, "cpu").items()}
    return out


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("name", ["r17", "above"])
def test_device_against_the_host_mirror(name, dt, mirror):
    shape, ranks = ([33, 33, 33], [17, 17]) if name == "r17" else ([2, 2, 2], [_hip.mode_sandwich_max_rank() + 1] * 2)
    cores, marg = _random_train(shape, ranks, dt, 7)
    t = tn.Tensor([c.cuda() for c in cores])
    marg = [m.cuda() for m in marg]
    for k, m in _masks(3, dt, "cuda").items():
        r = tn.sobol(t, m, marg)
        _on_device(r, dt)
        err = float(abs(ac.value(r) - mirror[name][k]).max())
        print(name, k, dt, "abs. error against the fp64 host mirror", err)
        assert err < (1e-4 if dt == torch.float32 else 1e-10), (name, k, err)


def test_mean_far_above_the_variance_fp32():
    """The golden train plus the constant 1000 (block cores), fp32: the indices do not move, and stay within 1e-4 of the fp64
    truth.  total - mean^2 in fp32 would be 1e6 2^-24 = 0.06 against a variance of 0.5."""
    t = ac.plus_constant(ac.train("t", torch.float32, "cuda"), 1000.0)
    w = ac.marginals(torch.float32, "cuda")
    for m in ac.MASKS:
        r = tn.sobol(t, ac.train("mask_" + m, torch.float32, "cuda"), w)
        err = ac.abs_err(r, "sobol_" + m)
        print("offset 1000,", m, "abs. error", err)
        assert err < 1e-4, (m, err)
    err = ac.abs_err(tn.sobol(t, ac.train("mask_true", torch.float32, "cuda"), w, normalize=False), "sobol_true_raw")
    print("offset 1000, total variance, abs. error", err)
    assert err < 1e-4


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "fp64"])
def test_decomposition_and_truncation_on_the_device(dt):
    t, w = ac.train("k", dt, "cuda"), ac.marginals(dt, "cuda", "kmarg")
    a = tn.anova_decomposition(t, w)
    assert all(U.is_cuda and U.dtype == dt for U in a.Us) and all(c.is_cuda for c in a.cores)
    back = tn.undo_anova_decomposition(a)
    full = t.torch()
    assert float((back.torch() - full).abs().max()) <= (1e-12 if dt == torch.float64 else 1e-6) * float(full.abs().max())
    t4 = ac.train("t", dt, "cuda")
    x = tn.symbols(4, dtype=dt, device="cuda")
    one = tn.truncate_anova(t4, tn.only(x[1]))
    assert one.dim() == 1 and one.cores[0].is_cuda and one.cores[0].dtype == dt
    assert ac.rel_err(one, "truncate_only_x1") < (1e-12 if dt == torch.float64 else 5e-6)
    keep = tn.truncate_anova(t4, tn.only(x[1]), keepdim=True)
    assert tuple(keep.shape) == tuple(t4.shape)
    assert ac.rel_err(keep, "truncate_only_x1_keepdim") < (1e-12 if dt == torch.float64 else 5e-6)


def test_sobol_of_a_pce_surrogate():
    """The use the module exists for: a first-order index of a surrogate fitted on the device."""
    X, y = pc.noisy_problem(300, 3)
    m = tn.PCEInterpolator()
    m.fit(X.cuda(), y.cuda(), p=4, verbose=False)
    t = m.to_tensor(domain=64, verbose=False)
    s = tn.sobol(t, tn.only(tn.symbols(3)[0]))
    assert s.is_cuda and s.dim() == 0 and s.dtype == t.cores[0].dtype
    total = sum(float(tn.sobol(t, tn.only(x))) for x in tn.symbols(3))
    print("first-order indices sum to", total, "x0:", float(s))
    assert 0.0 <= float(s) <= 1.0 + 1e-9 and total <= 1.0 + 1e-9

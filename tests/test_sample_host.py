"""``tn.sample`` on the CPU (the host mirror of ``ttr_sample_step``) against tests/golden/sample_f64.npz, recorded from the
unmodified reference, plus the exact cases, the refusals, and what the header, the library and the documents must say."""
import ctypes
import os

import numpy as np
import pytest
import torch

import sample_cases as sc
import tntorch_amd as tn
from tntorch_amd import _hip, tools

ROOT = sc.ROOT


def train(name, dtype):
    return tn.Tensor(sc.cores(name, dtype))


@pytest.mark.parametrize("name", list(sc.CASES))
def test_fp64_equals_the_reference(name):
    cs = sc.cores(name)
    X = tn.sample(tn.Tensor(cs), sc.P_GOLDEN, seed=sc.SEED_GOLDEN)
    assert X.dtype == torch.int64 and tuple(X.shape) == (sc.P_GOLDEN, len(cs)) and X.device.type == "cpu"
    nd = sc.explained(X, sc.golden(name), cs, sc.thresholds(sc.P_GOLDEN, len(cs)), torch.float64)
    print(f"{name}: {nd} rows differ from the reference")
    assert nd == 0   # none is expected: the restated algorithm differs from the reference in 0 of 4096 rows in fp64


@pytest.mark.parametrize("name", list(sc.CASES))
def test_fp32_is_explained(name):
    cs = sc.cores(name, torch.float32)
    X = tn.sample(tn.Tensor(cs), sc.P_GOLDEN, seed=sc.SEED_GOLDEN)
    U = sc.thresholds(sc.P_GOLDEN, len(cs))
    print(f"{name}: {sc.explained(X, sc.golden(name), cs, U, torch.float32)} rows differ from the reference")
    assert bool(sc.valid(cs, X, U, torch.float32).all())


def test_golden_rows_are_valid():
    """``valid`` itself, on decisions known to be right: the reference's."""
    for name in sc.CASES:
        cs = sc.cores(name)
        assert bool(sc.valid(cs, sc.golden(name), sc.thresholds(sc.P_GOLDEN, len(cs)), torch.float64).all())
    X = sc.golden("pos").clone()
    X[7, 2] = (X[7, 2] + 3) % 6
    ok = sc.valid(sc.cores("pos"), X, sc.thresholds(sc.P_GOLDEN, 4), torch.float64)
    assert not bool(ok[7]) and int((~ok).sum()) == 1


def test_shape_dtype_and_empty():
    t = train("pos", torch.float64)
    X = tn.sample(t, 3, seed=0)
    assert X.dtype == torch.int64 and tuple(X.shape) == (3, 4) and X.device.type == "cpu"
    assert tuple(tn.sample(t).shape) == (1, 4)
    E = tn.sample(t, 0, seed=0)
    assert E.dtype == torch.int64 and tuple(E.shape) == (0, 4)
    assert tuple(tn.sample(t, np.int64(2)).shape) == (2, 4)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_one_mode_exact(dtype):
    """[0, 3, 0, 1]: q, its running sums (0, 3, 3, 4) and u T = 4 u are exact in either dtype."""
    t = tn.Tensor([torch.tensor([0.0, 3.0, 0.0, 1.0], dtype=dtype).reshape(1, 4, 1)])
    u = sc.thresholds(sc.P_GOLDEN, 1)
    X = tn.sample(t, sc.P_GOLDEN, seed=sc.SEED_GOLDEN)
    assert torch.equal(X[:, 0], torch.where(u[:, 0] < 0.75, 1, 3))
    assert set(X[:, 0].tolist()) == {1, 3}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_extreme_thresholds(dtype):
    """u = 0 takes the first position of positive mass, u = 1 - 2^-53 the last one, also before trailing zeros."""
    t = tn.Tensor([torch.tensor(v, dtype=dtype).reshape(1, -1, 1) for v in ([0.0, 0.0, 2.0, 1.0, 0.0, 0.0], [0.5, 0.0, 0.25], [1.0, 3.0, 5.0, 0.0])])
    U = torch.tensor([[0.0, 0.0, 0.0], [1 - 2.0 ** -53] * 3], dtype=torch.float64)
    X = tools._sample_from_thresholds(t, U)
    assert X.tolist() == [[2, 0, 0], [3, 2, 2]]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_weight_mask_members(dtype):
    """Random members of a mask's accepted set: small integers, exact arithmetic."""
    m = tn.weight_mask(6, 2)
    t = tn.Tensor([c.to(dtype) for c in m.cores])
    X = tn.sample(t, 2000, seed=1)
    assert X.min() >= 0 and X.max() <= 1 and bool((X.sum(dim=1) == 2).all())
    assert len({tuple(r) for r in X.tolist()}) == 15   # every one of the C(6, 2) strings turns up among 2000 draws


def test_seed_none_draws_from_torch():
    t = train("pos", torch.float64)
    torch.manual_seed(3)
    X = tn.sample(t, 257)
    torch.manual_seed(3)
    U = torch.rand((257, 4), dtype=torch.float64)
    assert torch.equal(X, tools._sample_from_thresholds(t, U))
    assert not torch.equal(X, tn.sample(t, 257))


def test_tucker_factors_are_contracted_and_kept():
    torch.manual_seed(4)
    t = tn.rand([8, 7, 6, 5], ranks_tt=4, ranks_tucker=3, dtype=torch.float64)
    cores = [c.clone() for c in t.cores]
    Us = [U.clone() for U in t.Us]
    assert all(U is not None for U in Us)
    X = tn.sample(t, 500, seed=2)
    d = t.decompress_tucker_factors()
    assert all(U is None for U in d.Us)
    assert torch.equal(X, tn.sample(d, 500, seed=2))
    assert X.max() > 2   # indices of the full modes, not of the Tucker ranks
    assert all(torch.equal(a, b) for a, b in zip(cores, t.cores)) and all(torch.equal(a, b) for a, b in zip(Us, t.Us))


def test_refusals():
    t = train("pos", torch.float64)
    cs = sc.cores("pos")
    with pytest.raises(ValueError):
        tn.sample(tn.Tensor([c[None].repeat(2, 1, 1, 1) for c in cs], batch=True), 2, seed=0)
    with pytest.raises(NotImplementedError):
        tn.sample(tn.Tensor([torch.ones(4, 2), torch.ones(4, 2), torch.ones(4, 2)]), 2, seed=0)   # CP cores
    with pytest.raises(ValueError):
        tn.sample(t, -1, seed=0)
    with pytest.raises(ValueError):
        tn.sample(t, 1.5, seed=0)
    with pytest.raises(ValueError):
        tn.sample(tn.Tensor([torch.zeros_like(c) for c in cs]), 4, seed=0)
    # every first-mode slice leaves a left vector along e_0, and the second fiber's row 0 is zero
    a = torch.zeros(1, 3, 2, dtype=torch.float64)
    a[0, :, 0] = torch.tensor([1.0, 2.0, 3.0])
    b = torch.zeros(2, 3, 1, dtype=torch.float64)
    b[1, :, 0] = 1.0
    with pytest.raises(ValueError):
        tn.sample(tn.Tensor([a, b]), 4, seed=0)
    bad = [c.clone() for c in cs]
    bad[2][1, 2, 3] = float("nan")
    with pytest.raises(ValueError):
        tn.sample(tn.Tensor(bad), 4, seed=0)
    with pytest.raises(ValueError):
        tools._sample_from_thresholds(t, torch.ones((2, 4), dtype=torch.float64))   # u = 1.0 is outside [0, 1)


def test_exported():
    assert "sample" in tn.tools.__all__ and tn.sample is tn.tools.sample
    assert "sample" in tn.__doc__
    assert not hasattr(tn, "sum") and not hasattr(tn, "mean") and not hasattr(tn.Tensor, "sum") and not hasattr(tn.Tensor, "mean")


def test_header_library_and_binding():
    with open(os.path.join(ROOT, "include", "ttround_hip.h")) as f:
        header = f.read()
    assert "int ttr_sample_max_rank(void);" in header and "int ttr_sample_step(int dtype, int64_t P, int64_t r, int64_t I, int64_t rn," in header
    assert _hip.ABI_VERSION == 17
    assert {"ttr_sample_step", "ttr_sample_max_rank"} <= set(_hip.EXPORTED_SYMBOLS)
    assert (_hip.SAMPLE_ZERO_TOTAL, _hip.SAMPLE_NONFINITE, _hip.SAMPLE_BAD_THRESHOLD) == (1, 2, 4)
    lib = _hip.lib()
    assert lib.ttr_sample_max_rank() >= 128
    assert hasattr(lib, "ttr_sample_step")
    with open(os.path.join(ROOT, "tntorch_amd", "csrc", "Makefile")) as f:
        assert "ttr_sample.hip" in f.read()


def test_documents():
    def text(*parts):
        with open(os.path.join(ROOT, *parts)) as f:
            return f.read()

    assert "tn.sample" in text("README.md")
    design = text("DESIGN.md")
    assert "\n## 23. " in design and "ttr_sample_step" in design.split("\n## 23. ")[1]
    assert "gen_sample_golden.py" in text("tools", "README.md")


_BUF = [(ctypes.c_double * 512)() for _ in range(7)]
_A = [ctypes.addressof(b) for b in _BUF]


def _step(dtype=0, P=4, r=3, I=5, rn=2, L=0, fiber=1, core=2, u=3, X=4, Lnew=5, flag=6, strides=(10, 2, 1), ldl=3, ldn=2):
    a = lambda k: None if k is None else _A[k]
    cs = (ctypes.c_int64 * 3)(*strides)
    return _hip.lib().ttr_sample_step(dtype, P, r, I, rn, a(L), ldl, a(fiber), a(core), cs, a(u), 1, a(X), 1, a(Lnew), ldn, a(flag), None)


@pytest.mark.skipif(torch.cuda.is_available(), reason="host addresses must not reach a launch on a real device")
def test_cabi_refusals_before_any_device_call():
    INVALID, UNSUPPORTED = _hip.E_INVALID, _hip.E_UNSUPPORTED
    big = _hip.sample_max_rank() + 1
    assert _step(dtype=7) == INVALID
    assert _step(P=-1) == INVALID
    assert _step(I=0) == INVALID
    assert _step(r=big, ldl=big) == INVALID and _step(rn=big, ldn=big) == INVALID
    for name in ("L", "fiber", "core", "u", "X", "flag"):
        assert _step(**{name: None}) == INVALID, name
        assert b"null pointer" in _hip.lib().ttr_last_error()
    assert _step(strides=(10, 2, 3)) == UNSUPPORTED and _step(strides=(-10, 2, 1)) == UNSUPPORTED
    assert _step(ldl=2) == UNSUPPORTED and _step(ldn=1) == UNSUPPORTED
    assert _step(P=0) == 0   # returns at once: nothing is launched

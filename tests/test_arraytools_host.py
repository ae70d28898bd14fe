"""The array tools (``tn.squeeze``, ``unsqueeze``, ``unbind``, ``cat``, ``transpose``, ``flip``, ``ttm``, ``pad``,
``generate_basis``, ``cumsum``) on CPU tensors, against tests/golden/arraytools_f64.npz (the unmodified reference, recorded by
tools/gen_arraytools_golden.py) and against dense torch truths the reference cannot give.  Tolerances: relative Frobenius
1e-12 in fp64 and 1e-5 in fp32, those of test_moments_host.py; the inputs are the fixture's fp64 cores rounded to the dtype."""
import sys

import numpy as np
import pytest
import torch

import arraytools_cases as ac
import tntorch_amd as tn

DTYPES = [torch.float64, torch.float32]
TOOLS_NAMES = ["squeeze", "unsqueeze", "cat", "transpose", "flip", "unbind", "ttm", "generate_basis", "pad"]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", ac.cases())
def test_golden(case, dt):
    T, A = ac.inputs(dt)
    snap = ac.snapshot(T, A)
    out = ac.CASES[case](tn, T, A)
    for x in (out if isinstance(out, list) else [out]):
        first = x.cores[0] if hasattr(x, "cores") else x
        assert first.dtype == dt and first.device.type == "cpu"
    err = ac.rel_err(ac.dense(out), ac.truth(case))
    print(case, dt, "relative error", err)
    assert err <= ac.tol(dt)
    assert ac.unchanged(T, A, snap)   # inputs are bit-unchanged


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", sorted(ac.DENSE_TRUTHS))
def test_dense_truth(case, dt):
    T, A = ac.inputs(dt)
    snap = ac.snapshot(T, A)
    out, truth = ac.DENSE_TRUTHS[case](tn, T, A)
    err = ac.rel_err(ac.dense(out), truth)
    print(case, dt, "relative error", err)
    assert err <= ac.tol(dt)
    assert ac.unchanged(T, A, snap)


@pytest.mark.parametrize("name", ac.BASES)
@pytest.mark.parametrize("shape", ac.BASIS_SHAPES)
def test_generate_basis_golden(name, shape):
    U = tn.generate_basis(name, shape)
    assert U.dtype == torch.float64 and U.device.type == "cpu" and tuple(U.shape) == shape
    want = ac.fixture()["basis_{}_{}x{}".format(name, *shape)]
    assert float(np.abs(U.numpy() - want).max()) <= 1e-12 * max(1.0, float(np.abs(want).max()))


@pytest.mark.parametrize("name", ac.BASES)
def test_generate_basis_orthonormal_has_unit_columns(name):
    U = tn.generate_basis(name, (7, 4), orthonormal=True)
    assert float((U.norm(dim=0) - 1).abs().max()) < 1e-14
    plain = tn.generate_basis(name, (7, 4))
    assert float((U - plain / plain.norm(dim=0)).abs().max()) < 1e-14


def test_dct_is_the_orthonormal_dct2():
    U = tn.generate_basis("dct", (8, 8))
    assert float((U.t() @ U - torch.eye(8, dtype=torch.float64)).abs().max()) < 1e-14


def test_fp64_cat_works_under_the_fp32_default():
    assert torch.get_default_dtype() == torch.float32
    T, _ = ac.inputs(torch.float64)
    out = tn.cat([T["p"], T["q"]], dim=1)
    assert all(c.dtype == torch.float64 for c in out.cores)
    assert ac.rel_err(ac.dense(out), ac.truth("cat_pq_1")) <= 1e-12


def test_cat_of_one_is_a_clone():
    T, _ = ac.inputs(torch.float64)
    out = tn.cat([T["k"]], dim=0)
    assert out is not T["k"] and all(a is not b and torch.equal(a, b) for a, b in zip(out.cores, T["k"].cores))
    assert torch.equal(out.Us[0], T["k"].Us[0]) and out.Us[0] is not T["k"].Us[0]


@pytest.mark.parametrize("dt", DTYPES)
def test_reduce_with_cat(dt):
    out, truth = ac.reduce_cat(tn, dt)
    assert ac.rel_err(ac.dense(out), truth) <= (1e-5 if dt == torch.float32 else 1e-12)


def test_ranks_of_cat_add_and_pad_grows_by_at_most_two():
    T, _ = ac.inputs(torch.float64)
    p, q = T["p"], T["q"]
    for dim, ts in ((1, [p, q]), (1, [p, q, p]), (0, [p, p]), (2, [p, p])):
        want = [1] + [sum(int(t.ranks_tt[n]) for t in ts) for n in (1, 2)] + [1]
        assert tn.cat(ts, dim=dim).ranks_tt.tolist() == want
    stacked = tn.cat([T["k"], T["k"]], dim=0)
    assert stacked.Us[0] is not None and tuple(stacked.Us[0].shape) == (12, 8) and tuple(stacked.cores[0].shape) == (1, 8, 4)
    mixed = tn.cat([T["k"], T["k"].decompress_tucker_factors()], dim=0)
    assert mixed.Us[0] is None and tuple(mixed.cores[0].shape) == (1, 12, 4)
    assert tn.pad(p, [4, 6, 5]).ranks_tt.tolist() == p.ranks_tt.tolist()
    padded = tn.pad(p, [4, 6, 5], fill_value=7)
    assert all(0 <= int(a) - int(b) <= 2 for a, b in zip(padded.ranks_tt, p.ranks_tt))
    assert padded.ranks_tt[0] == 1 and padded.ranks_tt[-1] == 1


def test_squeeze_of_all_singletons_is_a_scalar():
    g = torch.Generator().manual_seed(1)
    t = ac.rand_train([1, 1, 1], 2, g, torch.float64)
    out = tn.squeeze(t)
    assert torch.is_tensor(out) and out.dim() == 0
    assert abs(float(out) - float(ac.dense(t).reshape(()))) < 1e-14


def test_unsqueeze_positions_refer_to_the_result():
    T, _ = ac.inputs(torch.float64)
    assert tuple(tn.unsqueeze(T["p"], [0, 2]).shape) == (1, 3, 1, 4, 5)
    assert tuple(tn.unsqueeze(T["p"], -1).shape) == (3, 4, 5, 1)
    assert tuple(tn.unsqueeze(T["p"], 3).shape) == (3, 4, 5, 1)


def test_errors():
    T, A = ac.inputs(torch.float64)
    p, q, k, s = T["p"], T["q"], T["k"], T["s"]
    with pytest.raises(ValueError, match="To concatenate tensors, all must have the same shape along all but the given dim"):
        tn.cat([p, q], dim=0)
    for call in (lambda: tn.cat([p, p], dim=3), lambda: tn.cat([p, p], dim=-4), lambda: tn.cat([p, k], dim=0),
                 lambda: tn.cat([p, tn.Tensor([c.float() for c in p.cores])], dim=0),
                 lambda: tn.flip(p, 3), lambda: tn.flip(p, [1, 1]), lambda: tn.flip(p, [1, -2]),
                 lambda: tn.cumsum(p, 3), lambda: tn.cumsum(p, [0, 0]),
                 lambda: tn.squeeze(s, 1), lambda: tn.squeeze(s, 4), lambda: tn.squeeze(s, [0, 0]),
                 lambda: tn.unsqueeze(p, 4), lambda: tn.unsqueeze(p, [0, 0]), lambda: tn.unbind(p, 3),
                 lambda: tn.ttm(p, A["A1"], dim=0),                      # [6, 4] on a mode of 3
                 lambda: tn.ttm(p, A["A1"], dim=1, transpose=True),       # contracts 6 entries of a mode of 4
                 lambda: tn.ttm(p, A["w1"], dim=0), lambda: tn.ttm(p, A["A1"], dim=3), lambda: tn.ttm(p, [A["A1"], A["A1"]], dim=[1, 1]),
                 lambda: tn.ttm(p, [A["A1"], A["A1"]], dim=1), lambda: tn.ttm(p, torch.zeros(2, 3, 4), dim=0),
                 lambda: tn.pad(p, [2, 6, 5]), lambda: tn.pad(p, 3, dim=1), lambda: tn.pad(p, [4, 6], dim=[0, 1, 2]), lambda: tn.pad(p, 6, dim=3),
                 lambda: tn.pad(k, 5, dim=0),
                 lambda: tn.generate_basis("fourier", (4, 4)), lambda: tn.generate_basis("dct", (4,))):
        with pytest.raises(ValueError):
            call()
    batched = tn.Tensor([torch.rand(2, 1, 3, 2), torch.rand(2, 2, 4, 1)], batch=True)
    cp = tn.Tensor([torch.rand(3, 2), torch.rand(4, 2)])
    for f in (lambda t: tn.cat([t, t], dim=0), tn.transpose, lambda t: tn.flip(t, 0), lambda t: tn.cumsum(t, 0), tn.squeeze,
              lambda t: tn.unsqueeze(t, 0), lambda t: tn.unbind(t, 0), lambda t: tn.ttm(t, torch.rand(2, 3), dim=0),
              lambda t: tn.pad(t, 5, dim=0)):
        with pytest.raises(ValueError, match="Batched tensors are not supported"):
            f(batched)
        with pytest.raises(NotImplementedError):
            f(cp)


def test_exports_and_scope():
    for name in TOOLS_NAMES:
        assert name in tn.tools.__all__ and getattr(tn, name) is getattr(tn.tools, name), name
    assert "cumsum" in tn.ops.__all__ and tn.cumsum is tn.ops.cumsum
    assert not hasattr(tn, "cumprod") and not hasattr(tn, "sum") and not hasattr(tn, "mean")
    assert not hasattr(tn.Tensor, "sum") and not hasattr(tn.Tensor, "mean")
    for f in [getattr(tn, n) for n in TOOLS_NAMES] + [tn.cumsum]:
        assert "tools.py:" in f.__doc__ or "ops.py:" in f.__doc__, f.__name__   # the reference's lines
        assert "Unlike the reference" in f.__doc__, f.__name__


def test_the_package_does_not_import_scipy():
    import subprocess

    code = "import sys, tntorch_amd as tn; tn.generate_basis('dct', (4, 4)); sys.exit(1 if 'scipy' in sys.modules else 0)"
    assert subprocess.run([sys.executable, "-c", code], cwd=ac.ROOT).returncode == 0


def test_host_mirror_signatures():
    from tntorch_amd import _hostops

    X, w = ac.kernel_input((3, 5, 7), torch.float32)
    truth, _ = ac.scan_truth(X)
    assert torch.equal(_hostops.mode_scan(X), truth.float())
    big = torch.full((3, 7, 9), -77.0)
    assert _hostops.mode_scan(X, out=big[:, 1:6, 2:9]).data_ptr() == big[:, 1:6, 2:9].data_ptr()
    assert torch.equal(big[:, 1:6, 2:9], truth.float()) and int((big == -77.0).sum()) == big.numel() - X.numel()
    rt, _ = ac.reduce_truth(X, w, 0.2)
    assert float((_hostops.mode_reduce(X, w, 0.2).double() - rt).abs().max()) <= 2.0 ** -23 * float(rt.abs().max())
    assert torch.equal(_hostops.mode_reduce(X), _hostops.mode_reduce(X, torch.ones(5)))


# ---------------------------------------------------------------------------------------------- random small cases
def _draw(rng, g, dt, N=None, shape=None):
    N = int(rng.integers(1, 4)) if N is None else N
    shape = [int(rng.integers(1, 10)) for _ in range(N)] if shape is None else shape
    tucker = [n for n in range(N) if rng.integers(0, 2)]
    return ac.rand_train(shape, int(rng.integers(1, 4)), g, dt, tucker=tucker)


@pytest.mark.parametrize("seed", range(20))
def test_random_cat(seed):
    """As the reference's test_cat draws them: N in 1..3, sizes in 1..9, Tucker and plain inputs mixed."""
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    t1 = _draw(rng, g, torch.float64)
    N, dim = t1.dim(), int(rng.integers(0, t1.dim()))
    shape2 = list(t1.shape)
    shape2[dim] = int(rng.integers(1, 10))
    t2 = _draw(rng, g, torch.float64, N=N, shape=shape2)
    out = tn.cat([t1, t2], dim=dim)
    truth = np.concatenate([ac.dense(t1), ac.dense(t2)], axis=dim)
    assert ac.rel_err(ac.dense(out), truth) <= 1e-12
    assert tuple(out.shape) == truth.shape


@pytest.mark.parametrize("seed", range(20))
def test_random_cumsum(seed):
    rng = np.random.default_rng(100 + seed)
    g = torch.Generator().manual_seed(100 + seed)
    t = _draw(rng, g, torch.float64)
    dims = [n for n in range(t.dim()) if rng.integers(0, 2)] or [0]
    truth = torch.from_numpy(ac.dense(t))
    for d in dims:
        truth = truth.cumsum(d)
    assert ac.rel_err(ac.dense(tn.cumsum(t, dims)), truth.numpy()) <= 1e-12

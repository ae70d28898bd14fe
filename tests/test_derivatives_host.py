"""tntorch_amd/derivatives.py on CPU tensors (the host mirror of ttr_mode_diff / ttr_laplace_core and the environment recursion on
_hostops.hsum_step) against tests/golden/derivatives_f64.npz: the unmodified reference's results and the dense fp64 truth."""
import numpy as np
import pytest
import torch

import derivatives_cases as dc
import tntorch_amd as tn
from tntorch_amd import _hostops

F64 = torch.float64


def _rand_tt(shape, ranks, seed=0, dtype=F64):
    g = torch.Generator().manual_seed(seed)
    rs = [1] + list(ranks) + [1]
    return tn.Tensor([torch.rand(rs[n], s, rs[n + 1], generator=g, dtype=dtype) for n, s in enumerate(shape)])


def _stencil(I, b, periodic=False):
    S = np.zeros((I, I))
    if periodic:
        for i in range(I):
            S[i, (i + 1) % I] += 1.0
            S[i, (i - 1) % I] -= 1.0
    elif I > 1:
        for i in range(1, I - 1):
            S[i, i + 1], S[i, i - 1] = 1.0, -1.0
        S[0, 1] += 2.0
        S[0, 0] -= 2.0
        S[I - 1, I - 1] += 2.0
        S[I - 1, I - 2] -= 2.0
    return S / ((b[1] - b[0]) / (I + 1) * 2)


def _along(x, d, Mx):
    return np.moveaxis(np.tensordot(Mx, x, axes=(1, d)), 0, d)


# ---------------------------------------------------------------------------------------------- the golden quantities
@pytest.mark.parametrize("q", sorted(dc.TENSOR))
def test_tensor_valued_golden(q):
    out = dc.TENSOR[q](tn, F64, "cpu")
    assert isinstance(out, tn.Tensor)
    dc.check_tensor(q, out, F64)
    assert dc.rel_err(out.torch(), q, against=dc.ref(q)) < 2e-12   # and the reference's own result (itself within 1e-12 of the truth)


def test_dgsm_golden():
    nu = dc.dgsm(tn, F64, "cpu")
    assert nu.shape == (4,) and nu.dtype == F64
    assert dc.rel_err(nu, "dgsm_a") < 1e-10
    assert dc.rel_err(nu, "dgsm_a", against=dc.ref("dgsm_a")) < 1e-5


def test_active_subspace_golden():
    M = dc.as_matrix(tn, F64, "cpu")
    assert dc.rel_err(M, "as_M") < 1e-10
    assert torch.equal(M, M.t())
    w, v = dc.active_subspace(tn, F64, "cpu")
    assert w.dtype == F64 and v.dtype == F64 and w.shape == (4,) and v.shape == (4, 4)
    assert bool((w[:-1] >= w[1:]).all())   # descending
    assert dc.rel_err(w, "as_w") < 1e-10
    assert dc.rel_err(w, "as_w", against=dc.ref("as_w")) < 1e-5
    assert dc.rel_err(dc.align_signs(v), "as_v") < 1e-10
    assert dc.rel_err(dc.align_signs(v), "as_v", against=dc.ref("as_v")) < 1e-5


# ---------------------------------------------------------------------------------------------- laplacian structure
def test_laplacian_ranks_are_2r_and_equal_the_sum_of_partials():
    t = dc.train("a", F64)
    b = dc.bounds("a")
    lap = tn.laplacian(t, bounds=b)
    assert lap.ranks_tt.tolist() == [1, 6, 6, 6, 1] and all(U is None for U in lap.Us)
    s = tn.partial(t, 0, order=2, bounds=b[0])
    for n in range(1, 4):
        s = s + tn.partial(t, n, order=2, bounds=b[n])
    assert s.ranks_tt.tolist() == [1, 12, 12, 12, 1]
    d = s.torch()
    assert float((lap.torch() - d).abs().max()) < 1e-12 * float(d.abs().max())
    k = tn.laplacian(dc.train("k", F64), bounds=dc.bounds("k"))
    assert k.ranks_tt.tolist() == [1, 4, 1] and all(U is None for U in k.Us)   # Tucker factors contracted in: a plain TT
    assert tn.laplacian(dc.train("v", F64), bounds=dc.bounds("v")).ranks_tt.tolist() == [1, 1]


def test_laplace_core_blocks_of_the_mirror():
    g = torch.Generator().manual_seed(1)
    X = torch.rand(3, 5, 4, generator=g, dtype=F64)
    D = _hostops.mode_diff(X, 2, False, 0.7)
    first, mid, last = (_hostops.laplace_core(X, pos, False, 0.7) for pos in (0, 1, 2))
    assert first.shape == (3, 5, 8) and torch.equal(first[:, :, :4], X) and torch.equal(first[:, :, 4:], D)
    assert mid.shape == (6, 5, 8) and torch.equal(mid[:3], first) and torch.equal(mid[3:, :, 4:], X) and not mid[3:, :, :4].any()
    assert last.shape == (6, 5, 4) and torch.equal(last[:3], D) and torch.equal(last[3:], X)


# ---------------------------------------------------------------------------------------------- step counts
def test_environment_recursion_step_counts(monkeypatch):
    N = 6
    t = _rand_tt([4, 5, 3, 4, 5, 3], [2, 3, 2, 3, 2], seed=3)
    calls = {"hsum": 0, "kron": 0}
    real_hsum, real_kron = _hostops.hsum_step, _hostops.core_kron

    def hsum(*a, **kw):
        calls["hsum"] += 1
        return real_hsum(*a, **kw)

    def kron(*a, **kw):
        calls["kron"] += 1
        return real_kron(*a, **kw)

    monkeypatch.setattr(_hostops, "hsum_step", hsum)
    monkeypatch.setattr(_hostops, "core_kron", kron)
    b = [[0.0, 1.0 + n] for n in range(N)]
    w, v = tn.active_subspace(t, b)
    assert 0 < calls["hsum"] <= N * N + 3 * N and calls["kron"] == 0, calls
    calls["hsum"] = 0
    nu = tn.dgsm(t, b)
    assert 0 < calls["hsum"] <= 3 * N and calls["kron"] == 0, calls
    # and the values are those of the reference's algorithm written with this package's partial, * and dot
    monkeypatch.undo()
    grad = tn.gradient(t, bounds=b)
    pdf = tn.Tensor([torch.full((1, I, 1), 1.0 / I, dtype=F64) for I in t.shape])
    ref = torch.stack([tn.dot(gn * pdf, gn) for gn in grad])
    assert float((nu - ref).abs().max()) < 1e-12 * float(ref.abs().max())
    mid = tn.Tensor([torch.cat([torch.full((I - 1,), 1.0 / (I - 1), dtype=F64), torch.zeros(1, dtype=F64)])[None, :, None] for I in t.shape])
    M = torch.stack([tn.dot(grad[i] * mid, grad[j]) for i in range(N) for j in range(N)]).reshape(N, N)
    rw = torch.linalg.eigvalsh(M).flip(0)
    assert float((w - rw).abs().max()) < 1e-11 * float(rw.abs().max())


# ---------------------------------------------------------------------------------------------- documented differences
def test_default_bounds_are_per_mode():
    t = dc.train("a", F64)   # 5 x 6 x 7 x 4: unequal mode sizes
    a = t.torch().numpy()
    for d in range(4):
        out = tn.partial(t, d).torch().numpy()
        truth = _along(a, d, _stencil(a.shape[d], [0, a.shape[d]]))
        assert np.abs(out - truth).max() < 1e-12 * np.abs(truth).max(), d
    truth = sum(_along(a, d, np.linalg.matrix_power(_stencil(a.shape[d], [0, a.shape[d]]), 2)) for d in range(4))
    assert np.abs(tn.laplacian(t).torch().numpy() - truth).max() < 1e-12 * np.abs(truth).max()
    out = tn.partial(t, [1, 3]).torch().numpy()   # a list of modes: each takes its own extent
    truth = _along(_along(a, 1, _stencil(6, [0, 6])), 3, _stencil(4, [0, 4]))
    assert np.abs(out - truth).max() < 1e-12 * np.abs(truth).max()


def test_gradient_with_an_int_dim_passes_bounds_as_bounds():
    t = dc.train("a", F64)
    a = t.torch().numpy()
    out = tn.gradient(t, dim=1, bounds=[0, 2])
    assert isinstance(out, tn.Tensor)
    truth = _along(a, 1, _stencil(6, [0, 2]))
    assert np.abs(out.torch().numpy() - truth).max() < 1e-12 * np.abs(truth).max()
    both = tn.gradient(t, dim=[0, 2], bounds=[[0, 1], [0, 3]])
    assert isinstance(both, list) and len(both) == 2
    truth = _along(a, 2, _stencil(7, [0, 3]))
    assert np.abs(both[1].torch().numpy() - truth).max() < 1e-12 * np.abs(truth).max()


def test_marginals_are_not_modified():
    t = dc.train("a", F64)
    marg = dc.marginals(F64)
    keep = [m.clone() for m in marg]
    tn.dgsm(t, dc.bounds("a"), marg)
    tn.active_subspace(t, dc.bounds("a"), marg)
    assert all(torch.equal(m, k) for m, k in zip(marg, keep))


@pytest.mark.parametrize("dt", [torch.float32, F64])
def test_results_follow_the_dtype(dt):
    t = dc.train("a", dt)
    assert tn.partial(t, 1, bounds=[0, 1]).cores[1].dtype == dt
    assert tn.laplacian(t).cores[0].dtype == dt
    assert tn.dgsm(t, dc.bounds("a")).dtype == dt
    w, v = tn.active_subspace(t, dc.bounds("a"))
    assert w.dtype == dt and v.dtype == dt and w.device == t.cores[0].device
    if dt == torch.float32:
        assert dc.rel_err(dc.dgsm(tn, dt, "cpu"), "dgsm_a") < 1e-5


def test_refusals():
    t = dc.train("a", F64)
    f = [dc.train("f{}".format(n), F64) for n in range(3)]
    batched = tn.Tensor([torch.rand(2, 1, 4, 2), torch.rand(2, 2, 4, 1)], batch=True)
    cp = tn.Tensor([torch.rand(4, 3), torch.rand(5, 3)])
    for fn in (lambda x: tn.partial(x, 0), lambda x: tn.gradient(x), lambda x: tn.laplacian(x), lambda x: tn.dgsm(x, [0, 1]),
               lambda x: tn.active_subspace(x, [0, 1]), lambda x: tn.divergence([x, x]), lambda x: tn.curl([x, x, x])):
        with pytest.raises(ValueError):
            fn(batched)
        with pytest.raises(NotImplementedError):
            fn(cp)
    bad = [
        lambda: tn.partial(t, 0, order=0),
        lambda: tn.partial(t, 0, order=1.5),
        lambda: tn.partial(t, 4),
        lambda: tn.partial(t, -5),
        lambda: tn.partial(t, [0, 1], bounds=[[0, 1]]),
        lambda: tn.partial(t, [0, 1], periodic=[True]),
        lambda: tn.gradient(t, dim=[0, 1], bounds=[[0, 1], [0, 1], [0, 1]]),
        lambda: tn.gradient(t, dim=7),
        lambda: tn.laplacian(t, bounds=[[0, 1]] * 3),
        lambda: tn.dgsm(t, [[0, 1]] * 5),
        lambda: tn.dgsm(t, [0, 1], dc.marginals(F64)[:3]),
        lambda: tn.dgsm(t, [0, 1], [torch.ones(3)] * 4),
        lambda: tn.active_subspace(t, [[0, 1]] * 3),
        lambda: tn.active_subspace(t, [0, 1], dc.marginals(F64)[:2]),
        lambda: tn.divergence(f[:2]),
        lambda: tn.divergence(f, bounds=[[0, 1]] * 2),
        lambda: tn.divergence([f[0], f[1], _rand_tt([5, 5, 4], [2, 2])]),
        lambda: tn.curl(f[:2]),
        lambda: tn.curl([t, t, t]),
        lambda: tn.curl(f, bounds=[[0, 1]] * 4),
        lambda: tn.curl([f[0], f[1], _rand_tt([5, 4, 5], [2, 2])]),
    ]
    for n, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
            pytest.fail("case {} did not raise".format(n))


# ---------------------------------------------------------------------------------------------- small modes, Tucker factors
def test_mode_sizes_one_and_two():
    one = _rand_tt([3, 1, 4], [2, 2], seed=5)
    assert not tn.partial(one, 1, bounds=[0, 1]).torch().any()
    assert not tn.partial(one, 1, bounds=[0, 1], periodic=True).torch().any()
    two = _rand_tt([3, 2, 4], [2, 2], seed=6)
    x = two.torch().numpy()
    for per in (False, True):
        for order in (1, 2):
            truth = _along(x, 1, np.linalg.matrix_power(_stencil(2, [0, 3], per), order))
            out = tn.partial(two, 1, order=order, bounds=[0, 3], periodic=per).torch().numpy()
            assert np.abs(out - truth).max() <= 1e-12 * max(np.abs(truth).max(), 1.0), (per, order)
    assert np.abs(_stencil(2, [0, 3]) - np.array([[-1.0, 1.0], [-1.0, 1.0]])).max() == 0   # rows 0 and I-1: 2 (e1 - e0), over step = 2


def test_tucker_factors_survive_partial():
    k = dc.train("k", F64)
    out = tn.partial(k, 0, order=2, bounds=dc.bounds("k")[0])
    assert out.Us[0] is not None and out.Us[0].shape == k.Us[0].shape and out.Us[1] is None
    assert torch.equal(out.cores[0], k.cores[0]) and out.cores[0].data_ptr() != k.cores[0].data_ptr()
    assert not torch.equal(out.Us[0], k.Us[0])
    g = tn.gradient(k, bounds=dc.bounds("k"))
    assert g[0].Us[0] is not None and g[1].Us[0] is not None and torch.equal(g[1].Us[0], k.Us[0])


def test_orders_above_the_fused_limit_on_the_mirror():
    g = torch.Generator().manual_seed(2)
    X = torch.rand(2, 9, 3, generator=g, dtype=F64)
    S = _stencil(9, [0, 4])
    truth = np.einsum("ij,rjc->ric", np.linalg.matrix_power(S, 5), X.numpy())
    out = _hostops.mode_diff(X, 5, False, 1.0 / ((4.0 / 10) * 2)).numpy()
    assert np.abs(out - truth).max() < 1e-12 * np.abs(truth).max()
    buf = torch.full((2, 9, 8), -7.0, dtype=F64)
    _hostops.mode_diff(X, 5, False, 1.0 / ((4.0 / 10) * 2), out=buf[:, :, 2:5])
    assert np.abs(buf[:, :, 2:5].numpy() - truth).max() < 1e-12 * np.abs(truth).max()
    assert bool((buf[:, :, :2] == -7).all()) and bool((buf[:, :, 5:] == -7).all())


def test_abi_and_documents():
    import os
    import re

    from tntorch_amd import _hip

    assert _hip.ABI_VERSION == 17
    for name in ("ttr_mode_diff", "ttr_laplace_core", "ttr_mode_diff_max_order"):
        assert name in _hip.EXPORTED_SYMBOLS
    design = open(os.path.join(dc.ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 16\.", design, flags=re.M) and "ttr_laplace_core" in design
    readme = open(os.path.join(dc.ROOT, "README.md")).read()
    assert "tn.laplacian" in readme and "partialset" in readme

"""``PCEInterpolator`` and its helpers on CPU tensors: the mirrors of the two kernels against the definition written with loops,
``gram_schmidt`` against the orthonormality it promises (tolerance measured on the reference's own result), ``_lars.lars_path``
against scikit-learn's path, exact recovery of a polynomial, the recorded results of the unmodified reference
(tests/golden/pce_f64.npz, tools/gen_pce_golden.py), and every refusal."""
import ctypes
import re

import numpy as np
import pytest
import torch

import pce_cases as pc
import tntorch_amd as tn
from tntorch_amd import _hip, _hostops, _lars

U = 2.0 ** -53


def _fit(X, y, **kw):
    m = tn.PCEInterpolator()
    m.fit(X, y, verbose=False, **kw)
    return m


@pytest.fixture(scope="module")
def fitted():
    z = pc.fixture()
    return _fit(torch.tensor(z["X"]), torch.tensor(z["y"]), p=int(z["p"]), q=float(z["q"]), val_split=float(z["val_split"]),
                seed=int(z["seed"]))


@pytest.fixture(scope="module")
def recovered():
    X, y = pc.recovery_problem()
    return X, y, _fit(X, y, p=4)


# ---------------------------------------------------------------------------------------------- the mirrors of the kernels
@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
@pytest.mark.parametrize("shape", pc.HOST_SHAPES)
def test_mirrors_match_the_definition(shape, dt):
    P, N, S, C = shape
    Z, Psi, coords, coef, _, _ = pc.kernel_inputs(N, S, dt, P=P, C=C, seed=3)
    truth = pc.loops_design(Z.double().numpy(), Psi.double().numpy(), coords.numpy())
    vec, A = pc.truth_design(Z.double().numpy(), Psi.double().numpy(), coords.numpy())
    assert float(np.abs(vec - truth).max()) <= float(((2 * S + N + 4) * 2.0 ** -52 * A).max())   # the two statements of the truth agree
    M = _hostops.pce_design(Z, Psi, coords)
    assert M.dtype == dt and tuple(M.shape) == (P, C)
    err = np.abs(M.double().numpy() - truth)
    bound = pc.kernel_bound(N, S, 0, dt, truth, A)
    print("design", shape, dt, "largest error", float(err.max()), "largest excess", float((err - bound).max()))
    assert bool((err <= bound).all())
    y = _hostops.pce_predict(Z, Psi, coords, coef)
    ty, Ay = truth @ coef.double().numpy(), A @ np.abs(coef.double().numpy())
    erry = np.abs(y.double().numpy() - ty)
    boundy = pc.kernel_bound(N, S, C, dt, ty, Ay)
    print("predict", shape, dt, "largest error", float(erry.max()), "largest excess", float((erry - boundy).max()))
    assert y.dtype == dt and tuple(y.shape) == (P,) and bool((erry <= boundy).all())
    big = torch.full((P + 2, C + 3), -77.0, dtype=dt)
    assert _hostops.pce_design(Z, Psi, coords, out=big[1 : P + 1, 2 : C + 2]).data_ptr() == big[1 : P + 1, 2 : C + 2].data_ptr()
    assert torch.equal(big[1 : P + 1, 2 : C + 2], M) and int((big == -77.0).sum()) == big.numel() - P * C


def test_mirror_refuses_coordinates_outside_the_basis():
    Z, Psi, coords, coef, _, _ = pc.kernel_inputs(3, 4, torch.float64, P=5, C=6, seed=4)
    for bad in (4, -1):
        c = coords.clone()
        c[2, 1] = bad
        with pytest.raises(ValueError, match="outside"):
            _hostops.pce_design(Z, Psi, c)
        with pytest.raises(ValueError, match="outside"):
            _hostops.pce_predict(Z, Psi, c, coef)


# ---------------------------------------------------------------------------------------------- gram_schmidt
@pytest.mark.parametrize("dist", ["uniform", "normal"])
def test_gram_schmidt_is_orthonormal_under_the_empirical_measure(dist):
    """Psi^T H Psi = I with H the fp64 moment matrix of the samples.  The tolerance is 10 x the residual of the reference's own
    fp64 result on the same data (the leading S x S block of the recorded 6 x 6 one is its result for S), floored at the unit
    roundoff 2^-53, below which a deviation from the identity's 1 cannot be told from none.  Measured (S = 6): ours 1.0e-14 /
    3.3e-15, the reference's 6.9e-15 / 7.7e-15 (uniform / normal)."""
    z = pc.fixture()
    x, ref = z["gs_" + dist], z["gs_" + dist + "_Psi"]
    assert x.shape == (500,)
    V = x[:, None] ** np.arange(6)
    H = V.T @ V / len(x)
    resid = lambda Psi: float(np.abs(Psi.T @ H[: len(Psi), : len(Psi)] @ Psi - np.eye(len(Psi))).max())
    for S in range(1, 7):
        Psi = tn.gram_schmidt(torch.tensor(x), S)
        assert Psi.dtype == torch.float64 and tuple(Psi.shape) == (S, S)
        Psi = Psi.numpy()
        ours, theirs = resid(Psi), resid(ref[:S, :S])
        print("gram_schmidt", dist, S, "residual", ours, "the reference's", theirs)
        assert ours <= 10.0 * max(theirs, U)
        assert np.array_equal(Psi, np.triu(Psi)) and Psi[0, 0] == 1.0
    assert tn.gram_schmidt(torch.tensor(x).float(), 4).dtype == torch.float32


# ---------------------------------------------------------------------------------------------- LARS against scikit-learn
@pytest.mark.parametrize("P, N, p", pc.LARS_PROBLEMS)
def test_lars_path_follows_sklearn(P, N, p):
    import sklearn.linear_model

    X, y = pc.noisy_problem(P, N)
    m = _fit(X, y, p=p)
    M = _hostops.pce_design((X - m.X_mean) / m.X_std, m.Psis, m.allcoords)
    C = M.shape[1]
    assert 14 <= C <= 21
    sk = sklearn.linear_model.Lars(n_nonzero_coefs=C, fit_intercept=False, fit_path=True).fit(M.numpy(), y.numpy())
    top = float(np.abs(sk.coef_path_).max())
    for dt, tol in ((torch.float64, pc.LARS_TOL_F64), (torch.float32, pc.LARS_TOL_F32)):
        Md = M.to(dt)
        Gb = _hostops.pce_gram(Md, y.to(dt))
        assert Gb.dtype == dt and tuple(Gb.shape) == (C + 1, C)
        G, b = Gb[:C], Gb[C]
        G0, b0 = G.clone(), b.clone()
        path, active = _lars.lars_path(G, b, n_samples=P)
        assert torch.equal(G, G0) and torch.equal(b, b0)
        assert path.dtype == np.float64 and path.shape == (C, C + 1) and path.shape == sk.coef_path_.shape
        assert active == [int(a) for a in sk.active_]
        err = float(np.abs(path - sk.coef_path_).max())
        print("lars", (P, N, p), dt, "C", C, "largest difference / largest entry", err / top, "cond(G / P)", float(np.linalg.cond(G.double().numpy() / P)))
        assert err <= tol * top
    short, act = _lars.lars_path(G, b, n_samples=P, max_steps=5)
    assert short.shape == (C, 6) and act == active[:5] and float(np.abs(short - path[:, :6]).max()) <= 1e-13 * top


# ---------------------------------------------------------------------------------------------- exact recovery
def test_exact_recovery_in_fp64(recovered):
    X, y, m = recovered
    pred = m.predict(X)
    err = pc.rel(pred, y)
    print("exact recovery: relative error on the training points", err, "selected", int(m.coords.shape[0]), "of", int(m.allcoords.shape[0]))
    assert pred.dtype == torch.float64 and err <= pc.RECOVERY_TOL
    assert tuple(m.Psis.shape) == (3, 4, 4) and m.allcoef.shape[0] == m.allcoords.shape[0] and m.coef.shape[0] == m.coords.shape[0]
    assert torch.equal(m.allcoords[m.allcoef != 0], m.coords) and torch.equal(m.allcoef[m.allcoef != 0], m.coef)
    t = m.to_tensor(domain=16, eps=1e-10, verbose=False)
    assert list(t.shape) == [16, 16, 16] and all(U_ is not None for U_ in t.Us)
    onto = m.predict(pc.grid_points(m.bbox, 16, torch.float64))
    err = float(torch.norm(t.torch().reshape(-1) - onto) / torch.norm(onto))
    print("to_tensor against predict on the 16^3 grid", err)
    assert err <= pc.TENSOR_TOL
    grid = [torch.linspace(-0.9, 0.8, 5, dtype=torch.float64), torch.linspace(-0.5, 0.5, 4, dtype=torch.float64), torch.tensor([0.1, 0.7], dtype=torch.float64)]
    t2 = m.to_tensor(domain=grid, eps=1e-10, verbose=False)
    pts = torch.stack(torch.meshgrid(*grid, indexing="ij"), dim=-1).reshape(-1, 3)
    assert list(t2.shape) == [5, 4, 2] and pc.rel(t2.torch().reshape(-1), m.predict(pts)) <= pc.TENSOR_TOL


def test_fp32_follows_the_input_dtype():
    X, y = pc.recovery_problem(torch.float32)
    m = _fit(X, y, p=4)
    for t in (m.X_mean, m.X_std, m.Psis, m.coef, m.allcoef, m.predict(X)):
        assert t.dtype == torch.float32
    assert m.coords.dtype == torch.int64 and m.allcoords.dtype == torch.int64
    err = pc.rel(m.predict(X), y)
    print("exact recovery in fp32", err)
    assert err <= 1e-5    # (the reference reaches 4e-7 in fp32)
    t = m.to_tensor(domain=6, eps=1e-6, verbose=False)
    assert t.cores[0].dtype == torch.float32 and t.Us[0].dtype == torch.float32


def test_retrain_false_takes_the_path_column(recovered):
    X, y, full = recovered
    m = _fit(X, y, p=4, retrain=False)
    assert torch.equal(m.allcoords, full.allcoords) and m.allcoef.shape[0] == m.allcoords.shape[0]
    assert torch.equal(m.allcoords[m.allcoef != 0], m.coords)
    assert pc.rel(m.predict(X), y) <= 1e-6


def test_verbose_prints_the_reference_lines(capsys):
    X, y = pc.recovery_problem()
    m = tn.PCEInterpolator()
    m.fit(X, y, p=4)
    m.to_tensor(domain=4)
    out = capsys.readouterr().out
    for piece in ("PCE interpolation (p=4, q=0.75) of 400 points (360 train + 40 val) in 3D", "Hyperbolic truncation... done, we kept 19 / 64 candidates",
                  "Assembling a 400 X 19 design matrix... done", "Finding best nnz in LARS... done, val eps=", "Retraining at nnz=",
                  "done, training eps=", "Conversion to TT-Tucker format (rmax=200, eps=0.001)", "Sparse TT-SVD... done, rmax="):
        assert piece in out, piece


# ---------------------------------------------------------------------------------------------- the reference's recorded results
def test_fit_matches_the_reference(fitted):
    z = pc.fixture()
    m = fitted
    assert np.array_equal(m.allcoords.numpy(), z["allcoords"])                      # the same candidate set, in the same order
    assert np.array_equal(m.coords.numpy(), z["coords"])                            # the same selection, in the same order
    assert np.array_equal(np.array(m.bbox), z["bbox"])
    assert pc.rel(m.X_mean, z["X_mean"]) <= 4 * U and pc.rel(m.X_std, z["X_std"]) <= 4 * U
    dev = {"coef": pc.rel(m.coef, z["coef"]), "predict": pc.rel(m.predict(torch.tensor(z["Xtest"])), z["ytest"]),
           "dense": pc.rel(m.to_tensor(domain=8, eps=1e-10, verbose=False).torch(), z["dense"])}
    print("against the reference (relative 2-norm):", dev, "Psis, largest difference", float(np.abs(m.Psis.numpy() - z["Psis"]).max()))
    assert dev["coef"] <= pc.FIXTURE_COEF_TOL and dev["predict"] <= pc.FIXTURE_PREDICT_TOL and dev["dense"] <= pc.FIXTURE_DENSE_TOL
    assert z["ytest"].shape == (50,) and z["dense"].shape == (8, 8, 8)


def test_indexing_helpers_are_bit_equal_to_the_reference():
    z = pc.fixture()
    hX = torch.tensor(z["h_X"])
    domain = [torch.tensor(z["h_domain_{}".format(n)]) for n in range(3)]
    box = [(lo + 0.3, hi - 0.2) for lo, hi in ((0.0, 2.0), (-1.0, 3.0), (5.0, 6.0))]
    assert np.array_equal(np.array(tn.get_bounding_box(hX)), z["h_bbox"])
    assert np.array_equal(tn.features2indices(hX).numpy(), z["h_idx"])
    assert np.array_equal(tn.features2indices(hX, bbox=box, I=16).numpy(), z["h_idx16"])
    assert int(z["h_idx16"].min()) == 0 and int(z["h_idx16"].max()) == 15                # (values outside the box are clamped)
    got = tn.features2indices(hX, domain=domain)
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), z["h_idx_domain"])
    assert np.array_equal(tn.features2indices(hX.reshape(2, 3, 2, 3), domain=domain).numpy(), z["h_idx_domain"].reshape(2, 3, 2, 3))
    assert np.array_equal(tn.indices2features(torch.tensor(z["h_idx_domain"]), domain=domain).numpy(), z["h_feat_domain"])
    feat = tn.indices2features(torch.tensor(z["h_idx16"]), bbox=z["h_bbox"].tolist(), I=16)    # the grid in the default dtype
    assert feat.dtype == torch.get_default_dtype() and float((feat.double() - torch.tensor(z["h_feat"])).abs().max()) <= 1e-5
    default = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)     # the dtype the fixture was recorded under: the helper's own grid, bit for bit
    try:
        feat = tn.indices2features(torch.tensor(z["h_idx16"]), bbox=z["h_bbox"].tolist(), I=16)
    finally:
        torch.set_default_dtype(default)
    assert feat.dtype == torch.float64 and np.array_equal(feat.numpy(), z["h_feat"])


def test_empirical_marginals():
    X = torch.tensor([[0.1, 5.0], [0.9, 5.0], [0.45, 7.2], [2.0, 6.1]], dtype=torch.float32)
    domain = [torch.tensor([0.0, 1.0]), torch.tensor([5.0, 6.0, 7.0])]
    got = tn.empirical_marginals(X, domain)
    assert [g.dtype for g in got] == [torch.float32] * 2
    assert torch.equal(got[0], torch.tensor([0.5, 0.5])) and torch.equal(got[1], torch.tensor([0.5, 0.25, 0.25]))


# ---------------------------------------------------------------------------------------------- refusals
def test_invalid_arguments_raise_value_error(recovered):
    X, y, m = recovered
    bad = [dict(X=X[:, 0]), dict(X=X.long()), dict(X=X.half()), dict(y=y[:-1]), dict(q=1.5), dict(q=-0.1), dict(q=0), dict(val_split=0.001)]
    for kw in bad:
        args = dict(X=X, y=y, p=3, verbose=False)
        args.update(kw)
        with pytest.raises(ValueError):
            tn.PCEInterpolator().fit(**args)
    with pytest.raises(ValueError, match="matrix_size_limit"):
        tn.PCEInterpolator().fit(X, y, p=4, matrix_size_limit=1000, verbose=False)
    with pytest.raises(ValueError):
        m.to_tensor(domain=[torch.linspace(0, 1, 4)] * 2, verbose=False)
    with pytest.raises(ValueError):
        tn.features2indices(X, bbox=[(0.0, 1.0)] * 2)
    with pytest.raises(ValueError):
        tn.features2indices(X, domain=[torch.linspace(0, 1, 4)] * 4)
    with pytest.raises(ValueError):
        tn.features2indices(X.long())
    with pytest.raises(ValueError):
        tn.indices2features(torch.zeros(3, 3, dtype=torch.long), bbox=[(0.0, 1.0)] * 2)
    with pytest.raises(ValueError):
        tn.empirical_marginals(X, [torch.linspace(0, 1, 4)] * 2)


def test_limits_and_symbols():
    """The host-only limit queries and the refusal above them before any launch (no GPU is touched: the checks come first)."""
    L = _hip.lib()
    assert L.ttr_pce_max_order() >= 16 and L.ttr_pce_max_basis() >= 256
    assert _hip.pce_max_order() == L.ttr_pce_max_order() and _hip.pce_max_basis() == L.ttr_pce_max_basis()
    with open(_hip._HEADER) as f:
        header = f.read()
    for name in ("ttr_pce_design", "ttr_pce_predict", "ttr_pce_max_order", "ttr_pce_max_basis"):
        assert re.search(r"\bint\s+{}\s*\(".format(name), header) and name in _hip.EXPORTED_SYMBOLS
    S1, NS1 = L.ttr_pce_max_order() + 1, L.ttr_pce_max_basis() + 1
    buf = ctypes.create_string_buffer(64)   # never dereferenced: every call below is refused before a launch
    ptr = ctypes.addressof(buf)
    for dtype, P, N, S, C, ldm in ((0, 4, 2, S1, 3, 3), (1, 4, NS1, 1, 3, 3), (0, 0, 2, 2, 3, 3), (0, 4, 2, 2, 0, 3), (7, 4, 2, 2, 3, 3), (1, 4, 2, 2, 3, 2)):
        assert L.ttr_pce_design(dtype, P, N, S, C, ptr, N, 1, ptr, ptr, ptr, ldm, ptr, None) == _hip.E_INVALID
    assert L.ttr_pce_predict(0, 4, 2, S1, 3, ptr, 2, 1, ptr, ptr, ptr, ptr, ptr, None) == _hip.E_INVALID
    assert L.ttr_pce_predict(1, 4, 2, 2, 3, ptr, 2, 1, ptr, ptr, None, ptr, ptr, None) == _hip.E_INVALID
    assert b"ttr_pce_predict" in L.ttr_last_error()


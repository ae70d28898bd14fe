"""The tests of the selected-eigenpair tests (eigsel_cases.py), without a GPU: the plain references pass their own checkers at the
bounds the GPU tests use, the Sturm certifier accepts the analytic Toeplitz spectrum and refuses shifted values, the table of the
reference's errors still agrees with a fresh computation, and every checker refuses a deliberately damaged reference output --
a dropped reflector, the reflectors in forward order, a dropped rank-2 term, an eigenvalue moved by 4 delta, the (j+1)-th
eigenvalue in place of the j-th, a vector with two entries swapped, a vector supported across an exact split."""
import math

import numpy as np
import pytest
import torch

import eigsel_cases as ec
from eigsel_cases import ECase, unit

DT = pytest.mark.parametrize("dt", ec.DTYPES, ids=["f32", "f64"])
# (family, n) on which C_lambda was calibrated with the plain bisection
REF_CASES = [("toeplitz", 2), ("toeplitz", 3), ("toeplitz", 65), ("toeplitz", 200), ("negtoeplitz", 100), ("wilkinson", 129),
             ("split", 90), ("split_end", 90), ("graded", 100), ("indefinite", 65)]


def _np(t):
    return t.numpy()


# ------------------------------------------------------------------ families and tables
def test_families_are_fp32_exact_and_split_gaps_hold():
    for c in ec.SIZE_CASES + ec.SWEEP_CASES + ec.FULL_CASES + ec.SCALED_CASES + ec.MIXED_BATCH:
        for dt in ec.DTYPES:
            d, e = ec.ecase_de(c, dt)                       # (asserts fp32 exactness)
            assert len(d) == c.n and e[c.n - 1] == 0.0 and 1 <= c.k <= min(c.n, 64)
            if dt == torch.float32:
                assert np.isfinite(d.astype(np.float32)).all() and np.isfinite((e.astype(np.float32)) ** 2).all()
        if c.family.startswith("split"):
            own = ec.split_owner(c.n, c.family == "split_end")   # (asserts the 0.1 tnorm gap)
            assert len(own) == c.n
    d, e = ec.family("split", 129)
    assert e[0] == 0.0 and e[1] != 0.0
    d, e = ec.family("split_end", 129)
    assert e[129 - 2] == 0.0 and d[128] == -7.0 - 0.125
    assert ec.family("negtoeplitz", 9)[0].max() < 0 and ec.gershgorin(*ec.family("indefinite", 9))[:2] == (-2.0, 2.0)
    assert set(ec.tridiag_table_keys()) == set(ec.TRIDIAG_REF_U)


def test_reference_error_table_matches_a_fresh_computation():
    """TRIDIAG_REF_U holds what tridiag_ref does today, for every item the GPU tests reduce (both dtypes, all sizes)."""
    for key, row in ec.TRIDIAG_REF_U.items():
        fresh = ec.tridiag_ref_errors(*key)
        for a, b in zip(row, fresh):
            assert abs(a - b) <= 0.02 * max(a, b, 1.0), (key, row, fresh)


@DT
def test_tridiag_ref_passes_its_checker(dt):
    """Backward error, orthogonality and reflector normalisation of the plain reduction: the figures the bounds were
    planned around (backward <= 35 u up to n = 1023, orthogonality <= 14 u) and 8 u for tau v^T v - 2, which is two dot products and a
    division away from exact."""
    worst = [0.0, 0.0, 0.0]
    for key, row in ec.TRIDIAG_REF_U.items():
        if key[0] == ec.dt_name(dt):
            worst = [max(a, b) for a, b in zip(worst, row)]
    print(f"tridiag_ref {ec.dt_name(dt)}: worst backward {worst[0]:.3g} u, orthogonality {worst[1]:.3g} u, reflector {worst[2]:.3g} u")
    # (in fp64 the checker computes Q^T Q and v^T v in the precision of what it checks: its own n-term dot products add a few u)
    slack = 0.0 if dt == torch.float32 else 8.0
    assert worst[0] <= 35.0 and worst[1] <= 14.0 + slack and worst[2] <= 8.0 + slack
    # the layout: leading 1 stored, e[n-1] = tau[n-1] = 0, and an already tridiagonal input comes back as it is
    d0, e0 = ec.family("wilkinson", 9)
    out, d, e, tau = ec.tridiag_ref(ec.tridiag_dense(d0, e0), dt)
    assert np.array_equal(d, d0) and np.array_equal(e, e0) and not tau.any() and all(out[k, k + 1] == 1 for k in range(8))


# ------------------------------------------------------------------ eigenvalues
@DT
@pytest.mark.parametrize("fam,n", REF_CASES, ids=[f"{f}{n}" for f, n in REF_CASES])
def test_bisect_and_twisted_refs_pass_their_checkers(dt, fam, n):
    """Plain bisection is certified at 2 u tnorm (a quarter of C_lambda), the twisted vectors have residual <= 10 u tnorm and
    norm error <= 4 u."""
    k = min(n, 6)
    d, e = ec.family(fam, n)
    tn, u = ec.gershgorin(d, e)[2], unit(dt)
    lam = ec.bisect_ref(d, e, k, dt)
    assert np.all(np.diff(lam) <= 0)
    assert ec.certify_all(d, e, lam, 2.0 * u * tn) == []
    res, nrm = ec.eigvec_errors(d, e, lam, ec.twisted_ref(d, e, lam, dt))
    print(f"{fam} n={n} {ec.dt_name(dt)}: residual {res / u:.3g} u tnorm, norm {nrm / u:.3g} u")
    assert res <= 10.0 * u and nrm <= 4.0 * u
    # ... and inside the bounds the GPU test derives from them
    c = ECase(fam, n, k, 0)
    assert res * tn <= ec.residual_bound(c, dt) and nrm <= (n + 4) * u


@DT
def test_refs_on_zero_scalar_scaled_and_full_spectra(dt):
    u = unit(dt)
    d, e = ec.family("zero", 65)
    lam = ec.bisect_ref(d, e, 6, dt)
    assert np.abs(lam).max() <= 8.0 * ec.pivmin(e, dt)
    res, nrm = ec.eigvec_errors(d, e, lam, ec.twisted_ref(d, e, lam, dt))
    assert res <= ec.residual_bound(ECase("zero", 65, 6, 0), dt) and nrm <= 4 * u
    d, e = ec.family("scalar", 65)
    lam = ec.bisect_ref(d, e, 6, dt)
    assert np.abs(lam.astype(np.float64) - ec.SCALAR_C).max() <= 4 * u * abs(ec.SCALAR_C)
    for c in ec.SCALED_CASES + [ECase("toeplitz", 5, 5, 0), ECase("split", 5, 5, 0), ECase("graded", 64, 64, 0)]:
        d, e = ec.ecase_de(c, dt)
        tn = ec.gershgorin(d, e)[2]
        lam = ec.bisect_ref(d, e, c.k, dt)
        assert ec.certify_all(d, e, lam, 2.0 * u * tn) == [], c
        res, nrm = ec.eigvec_errors(d, e, lam, ec.twisted_ref(d, e, lam, dt))
        assert res <= 10.0 * u and nrm <= 4.0 * u, (c, res / u, nrm / u)


@pytest.mark.parametrize("n", [2, 3, 65, 200])
def test_certifier_on_the_analytic_toeplitz_spectrum(n):
    """lambda_j = 2 - 2 cos((n - j) pi / (n + 1)), j = 0 the largest: accepted at delta, refused when moved by 3 delta."""
    d, e = ec.family("toeplitz", n)
    for dt in ec.DTYPES:
        delta = ec.C_LAMBDA * unit(dt) * 4.0
        for j in sorted({0, 1, n // 2, n - 1}):
            lam = 2.0 - 2.0 * math.cos((n - j) * math.pi / (n + 1))
            assert ec.sturm_certify(d, e, lam, j, delta), (n, j, dt)
            assert not ec.sturm_certify(d, e, lam + 3 * delta, j, delta), (n, j, dt)
            assert not ec.sturm_certify(d, e, lam - 3 * delta, j, delta), (n, j, dt)
    # exactly zero pivots (T = [[2, -1], [-1, 2]] has 1 and 3; the shifts 2 and 3 give a zero first / last pivot): counted as
    # negative, i.e. the count is that of the eigenvalues <= the shift, and the certificate stays sound
    d2, e2 = ec.family("toeplitz", 2)
    assert ec.sturm_certify(d2, e2, 2.5, 0, 0.5) and ec.sturm_certify(d2, e2, 1.25, 1, 0.75) and not ec.sturm_certify(d2, e2, 1.25, 0, 0.75)


@DT
@pytest.mark.parametrize("fam", ["toeplitz", "split", "graded", "wilkinson"])
def test_certifier_refuses_moved_and_off_by_one_eigenvalues(dt, fam):
    n, k = 65, 6
    d, e = ec.family(fam, n)
    delta = ec.C_LAMBDA * unit(dt) * ec.gershgorin(d, e)[2]
    lam = ec.bisect_ref(d, e, k, dt).astype(np.float64)
    assert ec.certify_all(d, e, lam, delta) == []
    for j in range(k):
        for sign in (-4.0, 4.0):
            assert not ec.sturm_certify(d, e, lam[j] + sign * delta, j, delta), (fam, j, sign)
    if fam != "wilkinson":   # (its top pair agrees to rounding: the second largest IS the largest within delta)
        off = ec.bisect_ref(d, e, k, dt, idx_shift=1)
        assert ec.certify_all(d, e, off, delta) == list(range(k))
    else:
        off = ec.bisect_ref(d, e, k, dt, idx_shift=1)
        assert ec.certify_all(d, e, off, delta) == [1, 3, 5]


# ------------------------------------------------------------------ eigenvectors
@DT
def test_eigvec_checker_refuses_swapped_entries_and_split_leakage(dt):
    c = ECase("split", 65, 6, 0)
    d, e = ec.ecase_de(c, dt)
    tn, u = ec.gershgorin(d, e)[2], unit(dt)
    lam = ec.bisect_ref(d, e, c.k, dt)
    Z = ec.twisted_ref(d, e, lam, dt)
    own = ec.split_owner(c.n, False)
    bound = ec.residual_bound(c, dt)
    assert ec.eigvec_errors(d, e, lam, Z)[0] * tn <= bound
    for j in range(c.k):
        first, m = own[j]
        assert ec.outside_block_max(Z[:, j], first, m) == 0.0
        if m == 1:
            assert abs(Z[first, j]) == 1.0
        else:
            Zs = Z.copy()
            i = first + int(np.argmax(np.abs(Z[first:first + m - 1, j])))
            Zs[[i, i + 1], j] = Zs[[i + 1, i], j]
            res, nrm = ec.eigvec_errors(d, e, lam, Zs)
            assert res * tn > bound and nrm <= (c.n + 4) * u, (j, res)
        # a vector that leaks into another block: a visible leak fails the residual, an invisible one the support check
        other = next(f for f, _ in own if f != first)
        for leak in (0.25, 1e-12):
            Zl = Z.astype(np.float64).copy()
            Zl[other, j] = leak
            assert ec.outside_block_max(Zl[:, j], first, m) > 0.0
            if leak > 1e-3:
                Zl[:, j] /= np.linalg.norm(Zl[:, j])
                assert ec.eigvec_errors(d, e, lam, Zl)[0] * tn > bound
    Zn = Z.copy()
    Zn[:, 0] *= 1.0 + 4 * (c.n + 4) * u
    assert ec.eigvec_errors(d, e, lam, Zn)[1] > (c.n + 4) * u
    Zn[3, 1] = np.nan
    assert ec.eigvec_errors(d, e, lam, Zn) == (np.inf, np.inf)


# ------------------------------------------------------------------ reduction
@DT
@pytest.mark.parametrize("n,b", [(9, 0), (65, 1), (64, 2), (129, 0)])
def test_tridiag_checker_refuses_a_dropped_rank2_term_and_bad_reflectors(dt, n, b):
    A0 = ec.tridiag_operand(n, b, dt)
    bounds = ec.tridiag_bounds(dt, n, b)
    good = ec.tridiag_ref(_np(A0), dt)
    errs = ec.tridiag_errors(A0, *good)
    assert all(x <= y for x, y in zip(errs, bounds)), (errs, bounds)
    live = [k for k in range(n - 2) if good[3][k] != 0]
    step = live[len(live) // 2]
    bad = ec.tridiag_ref(_np(A0), dt, drop_term_at=step)
    assert ec.tridiag_errors(A0, *bad)[0] > bounds[0]
    # a tau that is off by 1e-3 of itself fails the reflector check and the orthogonality
    out, d, e, tau = (x.copy() for x in good)
    tau[step] *= 1.001
    r = ec.tridiag_errors(A0, out, d, e, tau)
    assert r[1] > bounds[1] and r[2] > bounds[2]
    # the leading entry is used as stored: a missing 1 shows
    out, d, e, tau = (x.copy() for x in good)
    out[step, step + 1] = 0.0
    assert ec.tridiag_errors(A0, out, d, e, tau)[2] > bounds[2]
    # one off-diagonal with the wrong sign
    out, d, e, tau = (x.copy() for x in good)
    e[step] = -e[step]
    assert ec.tridiag_errors(A0, out, d, e, tau)[0] > bounds[0]
    out[0, 1] = np.nan
    assert ec.tridiag_errors(A0, out, d, e, tau)[0] == float("inf")


# ------------------------------------------------------------------ back-transformation
@DT
@pytest.mark.parametrize("n,k", [(3, 1), (65, 17), (200, 5)])
def test_back_checker_refuses_a_dropped_reflector_and_the_forward_order(dt, n, k):
    A, tau = ec.random_reflectors(n, n + 3, 1, dt)
    A, tau = _np(A[0]), _np(tau[0])
    assert np.isnan(A[:, n:]).all() and all(np.isnan(A[r, :r + 1]).all() for r in range(n))
    g = torch.Generator().manual_seed(n + k)
    Z0 = _np((3.0 * torch.randn(n, k, dtype=torch.float64, generator=g)).to(dt))
    u = unit(dt)
    ref = ec.back_errors(A, tau, Z0, ec.back_ref(A, tau, Z0, dt))
    bound = ec.bound_u(ref / u) * u
    print(f"back_ref n={n} k={k} {ec.dt_name(dt)}: {ref / u:.3g} u max|Z|")
    assert np.isfinite(ref) and ref <= 0.25 * max(n, 8) * u
    live = [i for i in range(n - 1) if tau[i] != 0]
    assert len(live) >= (n - 1) // 2 and (n < 10 or len(live) < n - 1)      # (some steps are dead, most are not)
    assert ec.back_errors(A, tau, Z0, ec.back_ref(A, tau, Z0, dt, skip=live[len(live) // 2])) > bound
    if len(live) > 1:
        assert ec.back_errors(A, tau, Z0, ec.back_ref(A, tau, Z0, dt, forward=True)) > bound


@DT
@pytest.mark.parametrize("n", ec.EXACT_N)
def test_exact_reflector_set_is_exact_and_order_dependent(dt, n):
    A, tau = ec.exact_reflectors(n, n + 3, 2, dt)
    g = torch.Generator().manual_seed(n)
    Z0 = _np(torch.randint(-9, 10, (n, 17), generator=g).to(dt))
    for b in range(2):
        Ab, tb = _np(A[b]), _np(tau[b])
        truth = ec.back_truth(Ab, tb, Z0).astype(np.float64)
        assert np.array_equal(ec.back_ref(Ab, tb, Z0, dt).astype(np.float64), truth)
        assert np.array_equal(np.sort(np.abs(truth), axis=0), np.sort(np.abs(Z0.astype(np.float64)), axis=0))   # a signed permutation
        if n > 3 or b == 0:     # (n = 3, item 1: two sign flips of different rows, which commute)
            assert not np.array_equal(ec.back_ref(Ab, tb, Z0, dt, forward=True).astype(np.float64), truth)
        assert not np.array_equal(ec.back_ref(Ab, tb, Z0, dt, skip=n // 2).astype(np.float64), truth)
    assert not np.array_equal(ec.back_truth(_np(A[0]), _np(tau[0]), Z0), ec.back_truth(_np(A[1]), _np(tau[1]), Z0))

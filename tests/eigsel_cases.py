"""What the tests of the selected-eigenpair kernels (``ttr_eigsel.hip``: ``ttr_tridiag``, ``ttr_tri_eigsel``, ``ttr_tridiag_back``)
share: tridiagonal families, seeded operands, plain references in the working precision, a Sturm-count certifier in ``decimal``,
fp64 checkers and the case tables.  Importable without a GPU.  Each stage is held to its own mathematical contract:

  ttr_tridiag       A = Q T Q^T with Q = H_0 ... H_{n-2} rebuilt in fp64 from what the kernel left (row k of A, tau): the backward
                    error max|Q T Q^T - A| / max|A|, the orthogonality max|Q^T Q - I|, and max_k |tau_k v_k^T v_k - 2| (a reflector
                    I - tau v v^T is orthogonal iff tau v^T v = 2) over the steps with tau_k != 0 (`tridiag_errors`).
  ttr_tri_eigsel    lam[j] is PROVEN to be the j-th largest eigenvalue of the given T within delta by two Sturm counts evaluated in
                    80-digit decimal arithmetic on the exact rational inputs (`sturm_certify`): no eigensolver is the truth, so the
                    check holds for fp64 kernels as it does for fp32.  Vectors: max|T z - lam z| / tnorm and | ||z|| - 1 | in fp64
                    (`eigvec_errors`), tnorm = max(|gl|, |gu|) of the Gershgorin interval, the scale the kernel itself uses.
  ttr_tridiag_back  X = Q Z against the application of the same reflectors in extended precision (`back_errors`, `back_truth`:
                    long double, u = 2^-64 -- an fp64 truth could not judge an fp64 kernel); on the exact reflector set
                    (signed permutations, integer Z) the result is exact in both dtypes.

The bounds, with u the unit roundoff of the dtype (2^-24, 2^-53).  None is taken from a kernel's output.
  C_lambda = 8   delta = 8 u tnorm, independent of n.  The Sturm recurrence is backward stable entrywise (a few u tnorm) and the final
                 bracket of a bisection is at most 2 u tnorm wide; `bisect_ref` (plain bisection in the working precision) certifies
                 at 2 u tnorm on every family / size / dtype of `test_eigsel_cases_host.py`.  The factor 4 over that covers the
                 multisection's other shift placement and the fast reciprocal of the fp32 pivot division.
  tridiag        per case 4 x what `tridiag_ref` (unblocked Householder reduction, larfg convention, numpy's pairwise sums, working
                 precision) makes on the same input in the same dtype, floor 8 u, for each of the three `tridiag_errors`.  The 4
                 covers the summation order (wave trees there, pairwise / sequential here) and the kernels' fused update + product
                 pass.  The reference's errors are the constants of TRIDIAG_REF_U (units of u; `tridiag_ref_errors` recomputes
                 them and the host test asserts that the table still agrees): backward error up to 26 u at n = 1023, orthogonality
                 <= 7 u in fp32 and <= 20 u in fp64, where the fp64 checker's own rounding is part of the figure.
  C_r(n)         residual bound = max(8, 4 x `twisted_ref`'s residual on the same (d, e, k, dtype)) u tnorm, computed when the test
                 runs (`eigsel_ref_errors`, cached); reference residuals are <= 10 u tnorm for n <= 200.  For the all-zero matrix
                 tnorm = 0 and the residual is |lam| |z_i| <= |lam| <= 8 pivmin, so there (only) the bound is 8 pivmin.
  norm           | ||z|| - 1 | <= (n + 4) u: n squares summed, one square root, one scaling (Higham, section 3.1).
  zero / scalar  |lam| <= 8 pivmin for T = 0 (the widened Gershgorin bracket is +- 2.1 pivmin and pivots below pivmin are replaced
                 by -pivmin);  |lam - c| <= 4 u |c| for T = c I (the count is exact, the last bracket is <= 2 eps |c| wide, its
                 midpoint is rounded once).  pivmin = tiny max(1, max e^2) / eps as in the kernel (LAPACK stebz, over eps).
  C_b(n)         max(8, 4 x `back_ref`'s error on the same reflectors and Z) u max|Z|, computed when the test runs.
  spectra        both paths of ttr_tridiag against eigvalsh(A) in fp64: n x the backward-error bound x max|A| (Weyl's
                 inequality with ||E||_2 <= n max|E|).
  pipeline       A X - X Lambda after tridiag -> fp64 eigh of T -> back: `pipeline_bound` (derived there).

Scaling.  The kernels do not rescale: e^2 and every pivot must stay normal numbers.  With the nonzero entries of T between 2^-1 and
2^4 in magnitude a factor s is admissible when s^2 e^2 is normal at both ends (the binding condition: 2^-126 <= s^2 2^-2 and
s^2 2^8 < 2^127 in fp32, 2^-1022 and 2^1023 in fp64); a pivot next to an eigenvalue (eps s tnorm), e^2 / pivot (s / eps) and
pivmin = tiny s^2 e^2 / eps << u s tnorm ask for less.  That is |log2 s| <= 59 in fp32 and |log2 s| <= 507 in fp64.  Tested:
2^+-20 (fp32) and 2^+-200 (fp64), on `toeplitz` and `split`; nothing beyond the admissible range is tested -- the kernel does not
rescale, and that is a documented limit, not a bug.  (`graded` in fp32 lets e^2 underflow from row ~125 on: the couplings it
loses are below 2^-63 = 2^-39 u tnorm, far inside delta, and only the top of the spectrum is asked for.)

Exact splits.  `split` / `split_end` join blocks whose spectra (centres 10, 0, -7, 5, radius < 2) are at least 0.1 tnorm apart (the
generator asserts it from the blocks' fp64 eigenvalues).  Across an exact zero of e the twisted factorisation has l = u = 0, and
the twist lands in the block that owns the eigenvalue because every gamma of another block is a pivot of a matrix at distance
>= 0.1 tnorm >> sqrt(n) u tnorm from singular: the vector is EXACTLY zero outside the owning block, and a size-1 block returns a
signed unit vector.
"""
import collections
import decimal
import functools

import numpy as np
import torch

from gemm_cases import DTYPES, unit  # noqa: F401  (DTYPES re-exported for the tests)

NP = {torch.float32: np.float32, torch.float64: np.float64}
C_LAMBDA = 8.0
FLOOR, FACTOR = 8.0, 4.0


def dt_name(dt):
    return "f32" if dt == torch.float32 else "f64"


def bound_u(ref_u):
    """The bound (units of u) that goes with a reference error (units of u): 4 x, floor 8."""
    return max(FLOOR, FACTOR * ref_u)


# ------------------------------------------------------------------ tridiagonal families
FAMILIES = ["toeplitz", "negtoeplitz", "wilkinson", "split", "split_end", "graded", "scalar", "zero", "indefinite"]
SCALAR_C = -1.5
SCALE_LOG2 = {torch.float32: 20, torch.float64: 200}


def _split_layout(n, end):
    """[(first, size, centre, e inside)] of the blocks of `split` (1, n/3, 1, rest) / `split_end` (1, n/3, rest, 1)."""
    a = n // 3
    sizes = [1, a, n - 2 - a, 1] if end else [1, a, 1, n - 2 - a]
    centres = [10.0, 0.0, 5.0, -7.0] if end else [10.0, 0.0, -7.0, 5.0]
    out, first = [], 0
    for m, c in zip(sizes, centres):
        if m > 0:
            out.append((first, m, c, -0.875 if c == 0.0 else 0.75))
            first += m
    assert first == n
    return out


def family(name, n, log2_scale=0):
    """(d, e) as fp64 arrays of values that fp32 represents exactly, e[n-1] = 0, times 2^log2_scale."""
    i = np.arange(n, dtype=np.float64)
    d, e = np.zeros(n), np.zeros(n)
    if name in ("toeplitz", "negtoeplitz", "indefinite"):
        d[:] = {"toeplitz": 2.0, "negtoeplitz": -2.0, "indefinite": 0.0}[name]
        e[:] = 1.0 if name == "negtoeplitz" else -1.0
    elif name == "wilkinson":
        assert n % 2 == 1
        d[:] = np.abs(i - (n - 1) / 2)
        e[:] = 1.0
    elif name in ("split", "split_end"):
        for first, m, c, off in _split_layout(n, name == "split_end"):
            d[first:first + m] = c + 0.125 * ((np.arange(m) % 3) - 1)
            e[first:first + m - 1] = off
    elif name == "graded":
        d = (2.0 ** (-i / 2)).astype(np.float32).astype(np.float64)
        e[:n - 1] = (0.3 * np.sqrt(d[:-1] * d[1:])).astype(np.float32).astype(np.float64)
    elif name == "scalar":
        d[:] = SCALAR_C
    else:
        assert name == "zero", name
    e[n - 1] = 0.0
    assert np.array_equal(d.astype(np.float32).astype(np.float64), d) and np.array_equal(e.astype(np.float32).astype(np.float64), e)
    s = 2.0 ** log2_scale          # (exact; 2^+-200 is for fp64 only)
    return d * s, e * s


def gershgorin(d, e):
    """(gl, gu, tnorm) in fp64: the Gershgorin interval and tnorm = max(|gl|, |gu|), the scale the kernel works with."""
    d, e = np.asarray(d, np.float64), np.asarray(e, np.float64)
    n = len(d)
    rad = np.abs(np.concatenate([e[:n - 1], [0.0]])) + np.abs(np.concatenate([[0.0], e[:n - 1]]))
    gl, gu = float((d - rad).min()), float((d + rad).max())
    return gl, gu, max(abs(gl), abs(gu))


def pivmin(e, dt):
    fi = torch.finfo(dt)
    e = np.asarray(e, np.float64)
    return fi.tiny * max(1.0, float((e[:len(e) - 1] ** 2).max()) if len(e) > 1 else 1.0) / fi.eps


def tridiag_dense(d, e):
    d, e = np.asarray(d, np.float64), np.asarray(e, np.float64)
    n = len(d)
    return np.diag(d) + np.diag(e[:n - 1], 1) + np.diag(e[:n - 1], -1)


@functools.lru_cache(maxsize=None)
def split_owner(n, end):
    """For `split` / `split_end` of size n: [(first, size)] of the block that owns the j-th largest eigenvalue, j = 0 .. n-1.
    Asserts the gap of the module docstring: spectra of different blocks are at least 0.1 tnorm apart."""
    d, e = family("split_end" if end else "split", n)
    tn = gershgorin(d, e)[2]
    ev = []
    for first, m, _, _ in _split_layout(n, end):
        w = np.linalg.eigvalsh(tridiag_dense(d[first:first + m], np.concatenate([e[first:first + m - 1], [0.0]])))
        ev += [(float(x), first, m) for x in w]
    ev.sort(key=lambda t: -t[0])
    for a, b in zip(ev[:-1], ev[1:]):
        assert a[1] == b[1] or a[0] - b[0] >= 0.1 * tn, (n, end, a, b, tn)
    return [(first, m) for _, first, m in ev]


# ------------------------------------------------------------------ Sturm certifier
_DEC_PREC = 80
_DEC_ZERO_PIVOT = decimal.Decimal("-1e-100000")


def _count_below(dd, e2, x):
    """Number of eigenvalues of T below x: the negative pivots of the LDL^T factorisation of T - x I (Sylvester), an exactly zero
    pivot counted as negative."""
    cnt, q = 0, None
    for i, di in enumerate(dd):
        q = di - x if i == 0 else di - x - e2[i - 1] / q
        if q == 0:
            q = _DEC_ZERO_PIVOT
        if q < 0:
            cnt += 1
    return cnt


def sturm_certify(d, e, lam, j, delta):
    """True iff count_below(lam - delta) <= n-1-j and count_below(lam + delta) >= n-j for the tridiagonal matrix (d, e) taken as
    exact rationals: at most n-1-j eigenvalues lie below lam - delta and at least n-j below lam + delta, so the j-th largest
    (ascending index n-1-j) lies in [lam - delta, lam + delta].  80-digit decimal arithmetic; no eigensolver involved."""
    n = len(d)
    with decimal.localcontext() as ctx:
        ctx.prec = _DEC_PREC
        dd = [decimal.Decimal(float(x)) for x in d]
        e2 = [decimal.Decimal(float(x)) ** 2 for x in e[:n - 1]]
        lo = decimal.Decimal(float(lam)) - decimal.Decimal(float(delta))
        hi = decimal.Decimal(float(lam)) + decimal.Decimal(float(delta))
        return _count_below(dd, e2, lo) <= n - 1 - j and _count_below(dd, e2, hi) >= n - j


def certify_all(d, e, lams, delta):
    """[j for which sturm_certify fails] over lams[j], j = 0 .. len(lams)-1 (the Decimal conversion is done once)."""
    n = len(d)
    bad = []
    with decimal.localcontext() as ctx:
        ctx.prec = _DEC_PREC
        dd = [decimal.Decimal(float(x)) for x in d]
        e2 = [decimal.Decimal(float(x)) ** 2 for x in e[:n - 1]]
        dl = decimal.Decimal(float(delta))
        for j, lam in enumerate(lams):
            lm = decimal.Decimal(float(lam))
            if not (_count_below(dd, e2, lm - dl) <= n - 1 - j and _count_below(dd, e2, lm + dl) >= n - j):
                bad.append(j)
    return bad


# ------------------------------------------------------------------ plain references in the working precision (numpy)
def tridiag_ref(A, dt, drop_term_at=None):
    """Unblocked Householder reduction of the symmetric A (numpy, any float dtype; computed in NP[dt]) with LAPACK's larfg
    convention, from the textbook (Golub & Van Loan, algorithm 8.3.1): returns (A_out, d, e, tau) laid out as ttr_tridiag leaves
    them -- reflector k in row k, columns k+1 .., leading 1 stored.  Sums are numpy's (pairwise), no BLAS.
    drop_term_at = k damages step k on purpose (the w v^T half of its rank-2 update is left out): host tests only."""
    f = NP[dt]
    A = np.array(A, dtype=f)
    n = A.shape[0]
    out = A.copy()
    d, e, tau = np.zeros(n, f), np.zeros(n, f), np.zeros(n, f)
    half, one = f(0.5), f(1.0)
    for k in range(n - 1):
        d[k] = A[k, k]
        x = A[k + 1:, k].copy()
        alpha, ss = x[0], f(np.sum(x[1:] * x[1:], dtype=f))
        v = np.zeros(n - k - 1, f)
        v[0] = one
        if ss == 0:
            e[k], tau[k] = alpha, f(0)
        else:
            beta = f(-np.copysign(np.sqrt(alpha * alpha + ss), alpha))
            tau[k] = (beta - alpha) / beta
            v[1:] = x[1:] * (one / (alpha - beta))
            e[k] = beta
            A22 = A[k + 1:, k + 1:]
            p = tau[k] * np.sum(A22 * v[None, :], axis=1, dtype=f)
            w = p - (half * tau[k] * f(np.sum(p * v, dtype=f))) * v
            A22 -= v[:, None] * w[None, :]
            if drop_term_at != k:
                A22 -= w[:, None] * v[None, :]
        out[k, k + 1:] = v
    d[n - 1] = A[n - 1, n - 1]
    return out, d, e, tau


def _ref_setup(d, e, dt):
    f = NP[dt]
    d, e = np.asarray(d, np.float64).astype(f), np.asarray(e, np.float64).astype(f)
    n = len(d)
    gl, gu, tn = gershgorin(d, e)
    return f, d, e, n, f(gl), f(gu), f(tn), f(pivmin(e, dt))


def bisect_ref(d, e, k, dt, idx_shift=0):
    """The k largest eigenvalues (descending) by plain bisection on Sturm counts in the working precision, one bracket per
    eigenvalue (vectorised over them), until the bracket is at most 2 u tnorm + 2 pivmin wide.  idx_shift = 1 asks for the
    (j+1)-th largest instead of the j-th on purpose: host tests only."""
    f, d, e, n, gl, gu, tn, pm = _ref_setup(d, e, dt)
    e2 = e * e
    u = f(unit(dt))
    pad = f(2.1) * tn * f(2) * u * f(n) + f(2.1) * pm
    lo, hi = np.full(k, gl - pad, f), np.full(k, gu + pad, f)
    idx = n - 1 - np.arange(k) - idx_shift
    with np.errstate(all="ignore"):
        for _ in range(2000):
            mid = lo + (hi - lo) * f(0.5)
            if np.all((hi - lo <= f(2) * u * tn + f(2) * pm) | (mid <= lo) | (mid >= hi)):
                break
            q = d[0] - mid
            q = np.where(np.abs(q) < pm, -pm, q)
            cnt = (q < 0).astype(np.int64)
            for i in range(1, n):
                q = d[i] - mid - e2[i - 1] / q
                q = np.where(np.abs(q) < pm, -pm, q)
                cnt += q < 0
            above = cnt >= idx + 1
            hi = np.where(above, mid, hi)
            lo = np.where(above, lo, mid)
    return (lo + (hi - lo) * f(0.5)).astype(f)


def twisted_ref(d, e, lam, dt):
    """Unit eigenvectors Z [n, k] for the eigenvalue approximations lam [k] from the twisted factorisation of T - lam I (Parlett &
    Dhillon's getvec: stationary qd transforms from both ends, the twist where |gamma| is smallest), in the working precision,
    pivots below pivmin replaced by -pivmin."""
    f, d, e, n, _, _, _, pm = _ref_setup(d, e, dt)
    lam = np.asarray(lam).astype(f)
    k = len(lam)
    Dp, L, U, Dm = (np.zeros((n, k), f) for _ in range(4))
    with np.errstate(all="ignore"):
        q = d[0] - lam
        for i in range(n - 1):
            q = np.where(np.abs(q) < pm, -pm, q)
            Dp[i], L[i] = q, e[i] / q
            q = d[i + 1] - lam - L[i] * e[i]
        Dp[n - 1] = q
        q = d[n - 1] - lam
        Dm[n - 1] = q
        for i in range(n - 2, -1, -1):
            q = np.where(np.abs(q) < pm, -pm, q)
            U[i] = e[i] / q
            q = d[i] - lam - U[i] * e[i]
            Dm[i] = q
        gam = Dp + Dm - (d[:, None] - lam[None, :])
        gam[n - 1] = Dp[n - 1]
        r = np.argmin(np.abs(gam), axis=0)
        Z = np.zeros((n, k), f)
        for c in range(k):
            z = Z[:, c]
            z[r[c]] = f(1)
            for i in range(r[c] - 1, -1, -1):
                z[i] = -L[i, c] * z[i + 1]
            for i in range(r[c], n - 1):
                z[i + 1] = -U[i, c] * z[i]
            z *= f(1) / np.sqrt(np.sum(z * z, dtype=f))
    return Z


def back_ref(A, tau, Z, dt, skip=None, forward=False):
    """X = H_0 ... H_{n-2} Z in the working precision, the reflectors (row k of A from column k+1, leading 1 stored) applied one by
    one, last first.  skip = k leaves reflector k out, forward = True applies them first to last: host tests only."""
    return _apply_reflectors(A, tau, Z, NP[dt], skip, forward)


def _apply_reflectors(A, tau, Z, f, skip=None, forward=False):
    n = Z.shape[0]
    X = np.array(Z, dtype=f)
    A, tau = np.asarray(A), np.asarray(tau)
    order = range(n - 1) if forward else range(n - 2, -1, -1)
    for k in order:
        if tau[k] == 0 or k == skip:
            continue
        v = A[k, k + 1:n].astype(f)
        dot = f(tau[k]) * np.sum(v[:, None] * X[k + 1:], axis=0, dtype=f)
        X[k + 1:] -= v[:, None] * dot[None, :]
    return X


# ------------------------------------------------------------------ checkers in fp64
def tridiag_errors(A0, A_out, d, e, tau):
    """(backward error max|Q T Q^T - A0| / max|A0|, max|Q^T Q - I|, max_k |tau_k v_k^T v_k - 2| over tau_k != 0) in fp64, Q = H_0
    ... H_{n-2} rebuilt from row k of A_out (columns k+1 .., the stored leading entry used as stored) and tau.  Torch tensors or
    numpy arrays of one matrix, on any device (the arithmetic runs where A_out lives)."""
    A_out = torch.as_tensor(A_out)
    dev = A_out.device
    cv = lambda x: torch.as_tensor(x).to(dev).double()  # noqa: E731
    A0, A_out, d, e, tau = cv(A0), cv(A_out), cv(d), cv(e), cv(tau)
    n = A0.shape[0]
    Q = torch.eye(n, dtype=torch.float64, device=dev)
    refl = torch.zeros((), dtype=torch.float64, device=dev)
    for k, t in reversed(list(enumerate(tau.tolist()[:n - 1]))):
        if t == 0.0:
            continue
        v = A_out[k, k + 1:]
        refl = torch.maximum(refl, (t * (v @ v) - 2.0).abs())
        S = Q[k + 1:, k + 1:]
        S -= torch.outer(t * v, v @ S)
    T = torch.diag(d) + torch.diag(e[:n - 1], 1) + torch.diag(e[:n - 1], -1)
    back = (Q @ T @ Q.T - A0).abs().max() / A0.abs().max().clamp_min(torch.finfo(torch.float64).tiny)
    orth = (Q.T @ Q - torch.eye(n, dtype=torch.float64, device=dev)).abs().max()
    nan_to_inf = lambda x: float("inf") if x != x else x  # noqa: E731
    return tuple(nan_to_inf(float(x)) for x in (back, orth, refl))


def eigvec_errors(d, e, lam, Z):
    """(max|T z - lam z| / tnorm, max| ||z|| - 1 |) over the columns of Z [n, k] in fp64; a zero tnorm leaves the residual
    unscaled."""
    d, e, lam, Z = (np.asarray(x, np.float64) for x in (d, e, lam, Z))
    n = len(d)
    R = d[:, None] * Z - Z * lam[None, :]
    R[:n - 1] += e[:n - 1, None] * Z[1:]
    R[1:] += e[:n - 1, None] * Z[:n - 1]
    tn = gershgorin(d, e)[2]
    with np.errstate(all="ignore"):
        res = float(np.abs(R).max()) / (tn if tn > 0 else 1.0)
        nrm = float(np.abs(np.sqrt((Z * Z).sum(axis=0)) - 1.0).max())
    return (res if res == res else np.inf), (nrm if nrm == nrm else np.inf)


def outside_block_max(z, first, size):
    """max |z_i| over the rows outside [first, first + size)."""
    z = np.asarray(z, np.float64)
    return float(np.abs(np.concatenate([z[:first], z[first + size:], [0.0]])).max())


def back_truth(A, tau, Z):
    """X = H_0 ... H_{n-2} Z from the same stored reflectors in numpy's long double (x87 extended precision, unit roundoff 2^-64).
    For fp32 that is as good as an fp64 application; for fp64 an fp64 application would BE back_ref, its error zero by
    construction and every bound the floor -- so the truth is taken 2^11 times finer than what it judges."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "back_truth needs an extended-precision long double"
    return _apply_reflectors(A, tau, Z, np.longdouble)


def back_errors(A, tau, Z0, X, truth=None):
    """max|X - truth| / max|Z0| against the extended-precision application of the same reflectors (back_truth)."""
    X64 = back_truth(A, tau, Z0) if truth is None else truth
    err = np.abs(np.asarray(X, np.longdouble) - X64).max() / np.abs(np.asarray(Z0, np.float64)).max()
    return float(err) if err == err else np.inf


# ------------------------------------------------------------------ operands of ttr_tridiag
KINDS = ["sym", "graded", "lowrank"]


def tridiag_kind(b):
    return KINDS[b % 3]


def tridiag_operand(n, b, dt):
    """Item b of size n (torch, dt): b % 3 = 0 symmetric indefinite randn + randn^T; 1 a graded Gram matrix (row scales 2^0 ..
    2^-7); 2 a Gram matrix of rank n / 2 whose trailing rows and columns are exactly zero.  The Gram factors are multiples of
    1/8, so the fp64 Gram matrix is exact whatever the order of its sums, and the operand is the same on every machine."""
    g = torch.Generator().manual_seed(1000 * n + b)
    kind = tridiag_kind(b)
    if kind == "sym":
        R = torch.randn(n, n, dtype=torch.float64, generator=g)
        return (R + R.T).to(dt)
    X = torch.round(torch.randn(n, n + 1, dtype=torch.float64, generator=g) * 8) / 8
    if kind == "graded":
        X = X * torch.ldexp(torch.ones(n, dtype=torch.float64), -((8 * torch.arange(n)) // n))[:, None]
    else:
        X[max(n // 2, 1):] = 0
    G = X @ X.T
    assert torch.equal(G, G.T)
    return G.to(dt)


GENERAL_N = [2, 3, 8, 9, 63, 64, 65, 127, 129, 200, 257]
PATHS_N = {torch.float32: [512, 513, 520, 1023], torch.float64: [512, 513]}
THRESHOLD_N = 512      # tridiag_spread: n >= 512 && batch <= 4


def tridiag_table_keys():
    """Every (dtype name, n, item) the GPU tests reduce."""
    keys = []
    for dt in DTYPES:
        keys += [(dt_name(dt), n, b) for n in GENERAL_N for b in range(3)]
        keys += [(dt_name(dt), n, b) for n in PATHS_N[dt] for b in range(5 if n == THRESHOLD_N else 2)]
    return keys


def tridiag_ref_errors(dtn, n, b):
    """`tridiag_errors` of `tridiag_ref` on item (n, b), in units of u."""
    dt = torch.float32 if dtn == "f32" else torch.float64
    A0 = tridiag_operand(n, b, dt)
    out = tridiag_ref(A0.numpy(), dt)
    return tuple(x / unit(dt) for x in tridiag_errors(A0, *out))


def tridiag_bounds(dt, n, b):
    """(backward, orthogonality, reflector) bounds of item (n, b) as absolute numbers."""
    return tuple(bound_u(r) * unit(dt) for r in TRIDIAG_REF_U[(dt_name(dt), n, b)])


# ------------------------------------------------------------------ cases of ttr_tri_eigsel
ECase = collections.namedtuple("ECase", "family n k scale")     # scale: -1 / 0 / +1 times SCALE_LOG2[dt]
EIGSEL_N = [2, 3, 5, 63, 64, 65, 129, 200]
SWEEP_K = [1, 2, 3, 5, 8, 9, 16, 17, 31, 32, 33, 63, 64]


def _fam_ok(fam, n):
    return fam != "wilkinson" or n % 2 == 1


SIZE_CASES = [ECase(fam, n, min(n, 6), 0) for fam in FAMILIES for n in EIGSEL_N if _fam_ok(fam, n)] + \
             [ECase(fam, 1024, 12, 0) for fam in ("toeplitz", "split")]
SWEEP_CASES = [ECase(fam, 129, k, 0) for fam in ("toeplitz", "split") for k in SWEEP_K]
FULL_CASES = [ECase(fam, n, n, 0) for fam in FAMILIES for n in (2, 3, 5, 64) if _fam_ok(fam, n)]
SCALED_CASES = [ECase(fam, 65, 6, s) for fam in ("toeplitz", "split", "split_end") for s in (-1, 1)]
MIXED_BATCH = [ECase(fam, 65, 5, 0) for fam in ("toeplitz", "graded", "split")]


def ecase_id(c):
    return f"{c.family}-n{c.n}-k{c.k}" + ("" if c.scale == 0 else ("-up" if c.scale > 0 else "-down"))


def ecase_de(c, dt):
    return family(c.family, c.n, c.scale * SCALE_LOG2[dt])


@functools.lru_cache(maxsize=None)
def eigsel_ref_errors(c, dt):
    """(residual / (u tnorm), norm error / u) of bisect_ref + twisted_ref on the case, in the dtype."""
    d, e = ecase_de(c, dt)
    lam = bisect_ref(d, e, c.k, dt)
    res, nrm = eigvec_errors(d, e, lam, twisted_ref(d, e, lam, dt))
    return res / unit(dt), nrm / unit(dt)


def residual_bound(c, dt):
    """The bound on max|T z - lam z| (absolute): max(8, 4 x reference) u tnorm; 8 pivmin for the zero matrix."""
    d, e = ecase_de(c, dt)
    tn = gershgorin(d, e)[2]
    if tn == 0.0:
        return 8.0 * pivmin(e, dt)
    return bound_u(eigsel_ref_errors(c, dt)[0]) * unit(dt) * tn


# ------------------------------------------------------------------ reflector sets for ttr_tridiag_back
BACK_N = [2, 3, 63, 64, 65, 127, 128, 129, 200, 1023, 1024]
BACK_K = [1, 15, 16, 17, 33, 64]
BACK_K_BIG = [1, 17]
EXACT_N, EXACT_K = [3, 64, 65, 130], [1, 17]


def back_ks(n):
    return BACK_K_BIG if n >= 1023 else BACK_K


def random_reflectors(n, lda, batch, dt, seed=0):
    """(A [batch, n, lda], tau [batch, n], Z [batch, n, k] drawn by the caller): row k of A holds v_k = (1, random) in columns k+1 ..
    n-1 and tau_k = 2 / ||v_k||^2 (rounded to dt: H_k is a reflector to rounding, which the fp64 truth shares); a seeded fifth of the
    steps has tau_k = 0 and a zero tail.  Every entry of row k at columns <= k, row n-1 and the padding columns n .. lda-1 are NaN:
    the kernel must never read them."""
    g = torch.Generator().manual_seed(77 * n + seed)
    A = torch.full((batch, n, lda), float("nan"), dtype=torch.float64)
    tau = torch.zeros((batch, n), dtype=torch.float64)
    for b in range(batch):
        dead = torch.rand(n, generator=g) < 0.2
        dead[0] = False
        for k in range(n - 1):
            v = torch.randn(n - 1 - k, dtype=torch.float64, generator=g).to(dt).double()
            v[0] = 1.0
            if dead[k]:
                v[1:] = 0.0
            else:
                tau[b, k] = 2.0 / float(v @ v)
            A[b, k, k + 1:n] = v
    return A.to(dt), tau.to(dt)


def exact_reflectors(n, lda, batch, dt):
    """Reflectors whose product is a signed permutation: even steps (where rows k+1, k+2 exist) v = (1, 1, 0, ...), tau = 1 -- H swaps
    the two rows and negates both -- odd steps v = (1, 0, ...), tau = 2 -- H flips the sign of row k+1.  Item b starts the
    alternation at step b.  On integer Z every operation is exact in both dtypes, and the product depends on the order."""
    A = torch.full((batch, n, lda), float("nan"), dtype=dt)
    tau = torch.zeros((batch, n), dtype=dt)
    for b in range(batch):
        for k in range(n - 1):
            A[b, k, k + 1:n] = 0.0
            A[b, k, k + 1] = 1.0
            if (k + b) % 2 == 0 and k + 2 < n:
                A[b, k, k + 2] = 1.0
                tau[b, k] = 1.0
            else:
                tau[b, k] = 2.0
    return A, tau


def pipeline_bound(n, k, dt, bt, bb, maxA, normA, maxZ):
    """Bound on ||A X - X Lambda||_F after ttr_tridiag (A = Q T Q^T + E, max|E| <= bt maxA), an fp64 eigh of T rounded to dt
    (Z, with T Z = Z Lambda to u) and ttr_tridiag_back (X = Q Z + F, max|F| <= bb maxZ):
        A X - X Lambda = Q (T Z - Z Lambda) + E X + (A - E) F - F Lambda,
    ||E||_F <= n max|E|, ||F||_F <= sqrt(n k) max|F|, ||X||_2 <= 1.01, ||Lambda||_2 <= ||A||_2 (1.01), ||T Z - Z Lambda||_F <=
    2.02 ||A||_2 sqrt(n k) u (every entry of Z is off by at most u) -- the sum of the two stage bounds and the rounding of Z."""
    rt = (n * k) ** 0.5
    return 1.01 * n * bt * maxA + 2.03 * normA * rt * bb * maxZ + 2.02 * normA * rt * unit(dt)


# ------------------------------------------------------------------ the reference's own errors (units of u), see tridiag_ref_errors
# (dtype, n, item) -> (backward, orthogonality, reflector)
TRIDIAG_REF_U = {
    ('f32', 2, 0): (0, 0, 0),
    ('f32', 2, 1): (0, 0, 0),
    ('f32', 2, 2): (0, 0, 0),
    ('f32', 3, 0): (7.378, 1.664, 0.8444),
    ('f32', 3, 1): (0.07921, 2.263, 1.174),
    ('f32', 3, 2): (0, 0, 0),
    ('f32', 8, 0): (3.63, 2.606, 1.566),
    ('f32', 8, 1): (2.96, 3.318, 2.021),
    ('f32', 8, 2): (0.9055, 0.4768, 0.251),
    ('f32', 9, 0): (3.344, 3.352, 2.259),
    ('f32', 9, 1): (8.183, 4.645, 2.641),
    ('f32', 9, 2): (5.386, 1.936, 1.318),
    ('f32', 63, 0): (9.3, 5.228, 4.757),
    ('f32', 63, 1): (4.376, 5.108, 4.267),
    ('f32', 63, 2): (5.951, 4.845, 5.289),
    ('f32', 64, 0): (5.817, 4.529, 4.269),
    ('f32', 64, 1): (10.01, 4.199, 3.692),
    ('f32', 64, 2): (5.269, 3.844, 3.6),
    ('f32', 65, 0): (7.843, 4.604, 3.848),
    ('f32', 65, 1): (4.765, 4.589, 3.749),
    ('f32', 65, 2): (9.398, 6.058, 3.946),
    ('f32', 127, 0): (8.299, 5.241, 4.562),
    ('f32', 127, 1): (9.687, 6.923, 4.719),
    ('f32', 127, 2): (8.659, 4.866, 4.482),
    ('f32', 129, 0): (9.943, 4.409, 3.586),
    ('f32', 129, 1): (10.89, 5.116, 4.585),
    ('f32', 129, 2): (12.96, 5.295, 4.721),
    ('f32', 200, 0): (8.178, 5.578, 5.299),
    ('f32', 200, 1): (6.4, 7.044, 5.888),
    ('f32', 200, 2): (9.969, 4.683, 3.495),
    ('f32', 257, 0): (8.278, 5.015, 4.44),
    ('f32', 257, 1): (10.2, 5.859, 5.153),
    ('f32', 257, 2): (11.13, 4.704, 4.626),
    ('f32', 512, 0): (15.27, 5.591, 5.877),
    ('f32', 512, 1): (9.163, 5.545, 5.339),
    ('f32', 512, 2): (13.32, 5.145, 5.169),
    ('f32', 512, 3): (11.57, 6.817, 6.36),
    ('f32', 512, 4): (9.969, 5.916, 4.902),
    ('f32', 513, 0): (14.09, 6.768, 5.522),
    ('f32', 513, 1): (11.64, 6.796, 5.856),
    ('f32', 520, 0): (19.47, 5.605, 5.572),
    ('f32', 520, 1): (13.54, 5.921, 5.206),
    ('f32', 1023, 0): (25.8, 6.164, 5.867),
    ('f32', 1023, 1): (17.83, 6.494, 5.018),
    ('f64', 2, 0): (0, 0, 0),
    ('f64', 2, 1): (0, 0, 0),
    ('f64', 2, 2): (0, 0, 0),
    ('f64', 3, 0): (8.405, 4, 4),
    ('f64', 3, 1): (0.06202, 1, 2),
    ('f64', 3, 2): (0, 0, 0),
    ('f64', 8, 0): (2.734, 6, 6),
    ('f64', 8, 1): (0.5416, 4, 4),
    ('f64', 8, 2): (2.61, 1.455, 2),
    ('f64', 9, 0): (5.701, 4, 4),
    ('f64', 9, 1): (5.596, 4, 4),
    ('f64', 9, 2): (4.109, 2.239, 4),
    ('f64', 63, 0): (9.753, 8, 8),
    ('f64', 63, 1): (12.35, 10, 6),
    ('f64', 63, 2): (5.512, 6, 6),
    ('f64', 64, 0): (7.865, 9, 6),
    ('f64', 64, 1): (7.47, 12, 8),
    ('f64', 64, 2): (9.203, 8, 4),
    ('f64', 65, 0): (10.14, 10, 6),
    ('f64', 65, 1): (18.99, 8, 6),
    ('f64', 65, 2): (9.983, 9, 4),
    ('f64', 127, 0): (13.3, 8, 8),
    ('f64', 127, 1): (10.88, 12, 8),
    ('f64', 127, 2): (13.57, 6, 8),
    ('f64', 129, 0): (13.44, 10, 8),
    ('f64', 129, 1): (24.93, 12, 6),
    ('f64', 129, 2): (11.04, 7, 4),
    ('f64', 200, 0): (12.81, 14, 8),
    ('f64', 200, 1): (10.2, 20, 10),
    ('f64', 200, 2): (12.39, 10, 6),
    ('f64', 257, 0): (12.81, 14, 8),
    ('f64', 257, 1): (17.53, 13, 8),
    ('f64', 257, 2): (11.99, 12, 8),
    ('f64', 512, 0): (18.52, 14, 10),
    ('f64', 512, 1): (23.6, 14, 12),
    ('f64', 512, 2): (16.77, 14, 8),
    ('f64', 512, 3): (18.54, 12, 12),
    ('f64', 512, 4): (22.99, 14, 10),
    ('f64', 513, 0): (20.39, 14, 8),
    ('f64', 513, 1): (16.2, 16, 10),
}

"""The selected-eigenpair kernels (ttr_eigsel.hip) through the raw C ABI on a real MI355X, stage by stage: ttr_tridiag (one
workgroup per matrix and the multi-launch "spread" path), ttr_tri_eigsel (Sturm-count multisection + twisted factorisation) and
ttr_tridiag_back, each against its own mathematical contract and at its edges -- n from 2, lda > n, batch strides, both reduction
paths at the same sizes and the batch threshold between them, every lane grouping of the multisection (G = 64 / kp, dead groups,
G = 1), k = n, negative / indefinite / exactly split / scaled spectra, the 16-wave column loop and the reflector order of the
back-transformation.

Method (eigsel_cases.py, whose docstring derives every bound): inputs are views inside NaN-filled buffers (padding columns, the
unused part of the reflector rows, the workspaces: a read outside the contract returns NaN), outputs lie inside sentinel-filled
buffers with 64 guard elements on either side which must keep their bits.  Eigenvalues are certified by Sturm counts in 80-digit
decimal arithmetic at delta = 8 u tnorm; the reduction, the vectors and the back-transformation are held to 4 x what a plain
working-precision reference makes on the same input (floor 8 u); exact data (tridiagonal / diagonal input, signed-permutation
reflectors, exact splits) must come back exactly.  Each test prints its worst error / bound ratio (`pytest -s`).

Worst error / bound seen on an MI355X (above 1 fails), fp32 / fp64:
  ttr_tridiag, n <= 257           0.39 / 0.64 (the fp64 maximum at n = 8, where the bound is the 8 u floor)
  both paths, n = 512 .. 1023     spread 0.35 / 0.39, one workgroup 0.37 / 0.36; spectra against eigvalsh(A) 3.8e-4 / 1.5e-2
  threshold, n = 512              batch 4 (spread) 0.29 / 0.39, batch 5 (one workgroup each) 0.32 / 0.46
  tridiagonal / diagonal input    d, e with equal bits, tau = 0, on both paths
  ttr_tri_eigsel                  every eigenvalue certified at 8 u tnorm (against fp64 LAPACK, printed only: 0.25 delta in fp32);
                                  residual 0.62 / 0.54, norm 0.19 / 0.33; split vectors exactly zero outside their block
  Wilkinson 129 through eigh_topk rmin = 0.0 (reported); graded and Toeplitz 1.0
  ttr_tridiag_back                random reflectors 0.36 / 0.36; signed permutations exact; pipeline 4.9e-3 / 9.4e-3
A build with the reflectors applied first to last, the Sturm index off by one, one partial-product chunk of the spread path left
out (when the support is 1 mod 256) and half of one step's rank-2 update dropped fails 88 of these 106 tests; what stays green
does not run the changed lines (n = 2, tau = 0 throughout, T = 0 or c I).
"""
import functools

import numpy as np
import pytest
import torch

import eigsel_cases as ec
import gemm_cases as gc
from eigsel_cases import unit
from gemm_cases import SENTINEL, Padded

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
DT = pytest.mark.parametrize("dt", ec.DTYPES, ids=["f32", "f64"])


def _hip():
    from tntorch_amd import _hip

    _hip.lib()
    return _hip


def call(name, *args):
    h = _hip()
    rc = getattr(h.lib(), name)(*args, h._stream())
    assert rc == 0, (name, rc, h.lib().ttr_last_error())
    torch.cuda.synchronize()


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def nan_bytes(nbytes):
    """A device buffer of all-ones bytes: NaN in fp32 and in fp64."""
    return torch.full((max(int(nbytes), 1),), 0xFF, dtype=torch.uint8, device=DEV)


def vec_out(B, n, dt):
    """A [B][n] output (d, e, tau, lam) inside a sentinel-filled buffer."""
    return Padded((1, B, n), dt, n, 0, SENTINEL, DEV)


def fetch(p, what):
    """The window of an output after a kernel ran; everything around it must have kept the fill's bits."""
    buf = p.buf.cpu()
    gc.assert_guards(p, buf, what)
    return p.view(buf).clone()


def report(group, what, ratio):
    print(f"ratio[{group}] {ratio:.3e}: {what}")


# ------------------------------------------------------------------ ttr_tridiag
def run_tridiag(mats, dt, ws=True, what=""):
    """ttr_tridiag on the stacked [n, n] matrices with lda = n + 3, strideA = n lda + 5, NaN around the squares: (A_out [B, n, n],
    d, e, tau [B, n], workspace written?).  The region outside the squares and around d / e / tau must keep its bits."""
    h = _hip()
    L = h.lib()
    code = h.dtype_code(dt)
    A0 = torch.stack(mats)
    B, n, _ = A0.shape
    a = Padded.of(A0, 3, 5, NAN, DEV)
    assert a.ld == n + 3 and a.stride == n * a.ld + 5
    d, e, tau = (vec_out(B, n, dt) for _ in range(3))
    wsb = L.ttr_tridiag_workspace_bytes(code, n, B)
    assert wsb >= B * 8 * n * (4 if dt == torch.float32 else 8)
    wbuf = nan_bytes(wsb)
    call("ttr_tridiag", code, n, B, a.ptr(), a.ld, a.stride, d.ptr(), e.ptr(), tau.ptr(), wbuf.data_ptr() if ws else None,
         wsb if ws else 0)
    touched = bool((wbuf != 0xFF).any())
    out = [fetch(p, f"{what} {name}") for p, name in ((a, "A"), (d, "d"), (e, "e"), (tau, "tau"))]
    return out[0], out[1][0], out[2][0], out[3][0], touched


def check_tridiag(group, dt, n, items, outs, what):
    """The three tridiag_errors of every item within 4 x the reference's (floor 8 u); e[n-1] = tau[n-1] = 0.  Row k of A at columns
    <= k is not looked at: ttr_tridiag_back reads row k from column k + 1 only, and the header promises nothing there."""
    A_out, d, e, tau, _ = outs
    worst = 0.0
    for i, b in enumerate(items):
        A0 = ec.tridiag_operand(n, b, dt)
        assert torch.isfinite(d[i]).all() and torch.isfinite(e[i]).all() and torch.isfinite(tau[i]).all(), (what, b)
        assert float(e[i, n - 1]) == 0.0 and float(tau[i, n - 1]) == 0.0, (what, b)
        dev = DEV if n >= 200 else "cpu"
        errs = ec.tridiag_errors(A0.to(dev), A_out[i].to(dev), d[i], e[i], tau[i])
        bounds = ec.tridiag_bounds(dt, n, b)
        ratios = [x / y for x, y in zip(errs, bounds)]
        worst = max(worst, *ratios)
        assert max(ratios) <= 1.0, (f"{what} item {b} ({ec.tridiag_kind(b)}): backward / orthogonality / reflector errors "
                                    f"{[x / unit(dt) for x in errs]} u, bounds {[x / unit(dt) for x in bounds]} u")
    report(group, what, worst)
    return worst


def tri_spectrum(d, e):
    return torch.linalg.eigvalsh(torch.as_tensor(ec.tridiag_dense(d.double().numpy(), e.double().numpy())))


@DT
@pytest.mark.parametrize("n", ec.GENERAL_N)
def test_tridiag_general(dt, n):
    """Batch 3 (symmetric indefinite, graded Gram, rank n/2 Gram with exactly zero trailing rows), lda = n + 3, strideA = n lda + 5."""
    what = f"tridiag n={n} {ec.dt_name(dt)}"
    mats = [ec.tridiag_operand(n, b, dt) for b in range(3)]
    outs = run_tridiag(mats, dt, ws=True, what=what)
    assert not outs[4], "the spread path is for n >= 512"
    check_tridiag("tridiag", dt, n, range(3), outs, what)
    # the rank-deficient item: the reduction meets zero columns, whose reflectors are H = I (tau = 0) with e = 0
    r = max(n // 2, 1)
    assert not outs[3][2, r:].any() and not outs[2][2, r:].any() and not outs[1][2, r:].any(), what
    # without a workspace: the same kernel, the same bits
    again = run_tridiag(mats, dt, ws=False, what=what + " (no workspace)")
    assert all(same_bits(x, y) for x, y in zip(outs[1:4], again[1:4])), what


@DT
@pytest.mark.parametrize("n,ws", [(2, False), (9, True), (65, False), (130, True), (513, True), (513, False)])
def test_tridiag_of_tridiagonal_and_diagonal_input_is_exact(dt, n, ws):
    """An input that is already tridiagonal (or diagonal): every reflector is H = I and every update term an exact zero -- d and e come
    back with equal bits, tau = 0 throughout.  n = 513 with a workspace takes the spread path (batch 2 per launch)."""
    # (graded only while 2^(-n/2) and its products with 0.3 are normal fp32 numbers)
    fams = [f for f in ec.FAMILIES if (f != "wilkinson" or n % 2 == 1) and (f != "graded" or n <= 200)]
    des = [ec.family(f, n) for f in fams] + [ec.family("toeplitz", n, ec.SCALE_LOG2[dt]), ec.family("split", n, -ec.SCALE_LOG2[dt])]
    des.append((np.resize(ec.family("graded", min(n, 130))[0], n), np.zeros(n)))      # diagonal, 130 different entries
    names = fams + ["toeplitz-up", "split-down", "diagonal"]
    for i0 in range(0, len(des), 2 if n >= 512 else len(des)):
        chunk = des[i0:i0 + (2 if n >= 512 else len(des))]
        mats = [torch.as_tensor(ec.tridiag_dense(d, e)).to(dt) for d, e in chunk]
        A_out, d, e, tau, touched = run_tridiag(mats, dt, ws=ws, what=f"exact n={n}")
        assert touched == (ws and n >= 512)
        for i, (d0, e0) in enumerate(chunk):
            what = f"{names[i0 + i]} n={n} {ec.dt_name(dt)}"
            assert same_bits(d[i], torch.as_tensor(d0).to(dt)), what
            assert same_bits(e[i], torch.as_tensor(e0).to(dt)), what
            assert not tau[i].any(), what
            assert all(float(A_out[i, k, k + 1]) == 1.0 for k in range(n - 1)), what     # the leading 1 is stored all the same


@pytest.mark.parametrize("dt,n", [(dt, n) for dt in ec.DTYPES for n in ec.PATHS_N[dt]],
                         ids=[f"{ec.dt_name(dt)}-{n}" for dt in ec.DTYPES for n in ec.PATHS_N[dt]])
def test_tridiag_both_paths(dt, n):
    """The same two matrices through the spread path (batch 2, workspace) and through one workgroup per matrix (workspace = NULL):
    both pass the checks of the general test, and the spectra of both T agree with eigvalsh(A) in fp64 within n x the backward-
    error bound x max|A| (Weyl; d and e themselves are not comparable between the paths)."""
    mats = [ec.tridiag_operand(n, b, dt) for b in range(2)]
    lam_ref = [torch.linalg.eigvalsh(m.double()) for m in mats]
    worst = 0.0
    for ws in (True, False):
        what = f"tridiag n={n} {ec.dt_name(dt)} {'spread' if ws else 'one workgroup'}"
        outs = run_tridiag(mats, dt, ws=ws, what=what)
        assert outs[4] == ws, what                            # the workspace is written by the spread path and by nothing else
        check_tridiag("tridiag-paths", dt, n, range(2), outs, what)
        for b in range(2):
            err = float((tri_spectrum(outs[1][b], outs[2][b]) - lam_ref[b]).abs().max())
            bound = n * ec.tridiag_bounds(dt, n, b)[0] * float(mats[b].abs().max())
            worst = max(worst, err / bound)
            assert err <= bound, (what, b, err, bound)
    report("tridiag-spectrum", f"n={n} {ec.dt_name(dt)}", worst)


@DT
@pytest.mark.parametrize("B", [4, 5])
def test_tridiag_spread_threshold(dt, B):
    """n = 512 with a workspace: batch 4 takes the spread path, batch 5 one workgroup per matrix."""
    n = ec.THRESHOLD_N
    what = f"tridiag n={n} batch {B} {ec.dt_name(dt)}"
    outs = run_tridiag([ec.tridiag_operand(n, b, dt) for b in range(B)], dt, ws=True, what=what)
    assert outs[4] == (B <= 4), what
    check_tridiag("tridiag-threshold", dt, n, range(B), outs, what)


# ------------------------------------------------------------------ ttr_tri_eigsel
def run_eigsel(des, k, dt, what=""):
    """ttr_tri_eigsel on the batch of (d, e): (lam [B, k], Z [B, n, k]) on the CPU; d / e inside NaN, the scratch handed over as NaN."""
    h = _hip()
    L = h.lib()
    code = h.dtype_code(dt)
    B, n = len(des), len(des[0][0])
    d = Padded.of(torch.as_tensor(np.stack([x[0] for x in des])).to(dt)[None], 0, 0, NAN, DEV)
    e = Padded.of(torch.as_tensor(np.stack([x[1] for x in des])).to(dt)[None], 0, 0, NAN, DEV)
    lam, Z = vec_out(B, k, dt), Padded((B, n, k), dt, k, n * k, SENTINEL, DEV)
    sb = L.ttr_eigsel_scratch_bytes(code, n, B)
    scratch = nan_bytes(sb)
    call("ttr_tri_eigsel", code, n, B, k, d.ptr(), e.ptr(), lam.ptr(), Z.ptr(), scratch.data_ptr(), sb)
    return fetch(lam, what + " lam")[0], fetch(Z, what + " Z")


def check_eigsel(c, dt, lam, Z, what):
    """One item: eigenvalues finite, descending, certified; vectors normalised, residual within C_r u tnorm; exact structure of
    the split / zero / scalar families.  Returns (eigenvalue error against fp64 LAPACK / delta -- printed only --, residual ratio,
    norm ratio)."""
    d, e = ec.ecase_de(c, dt)
    n, k, u = c.n, c.k, unit(dt)
    tn = ec.gershgorin(d, e)[2]
    lam64, Z64 = lam.double().numpy(), Z.double().numpy()
    assert np.isfinite(lam64).all() and np.isfinite(Z64).all(), what
    assert np.all(np.diff(lam64) <= 0), (what, lam64)
    delta = ec.C_LAMBDA * u * tn if tn > 0 else 8.0 * ec.pivmin(e, dt)
    bad = ec.certify_all(d, e, lam64, delta)
    assert bad == [], f"{what}: lam[j] is not the j-th largest eigenvalue within {delta:.3e} for j in {bad}: {lam64[bad]}"
    if c.family == "zero":
        assert np.abs(lam64).max() <= 8.0 * ec.pivmin(e, dt), (what, lam64)
    if c.family == "scalar":
        assert np.abs(lam64 - ec.SCALAR_C).max() <= 4.0 * u * abs(ec.SCALAR_C), (what, lam64)
    res, nrm = ec.eigvec_errors(d, e, lam64, Z64)
    rb = ec.residual_bound(c, dt)
    r_res, r_nrm = res * (tn if tn > 0 else 1.0) / rb, nrm / ((n + 4) * u)
    assert r_res <= 1.0, f"{what}: residual {res / u:.3g} u tnorm, bound {rb / (u * tn) if tn > 0 else rb:.3g}"
    assert r_nrm <= 1.0, f"{what}: | ||z|| - 1 | = {nrm / u:.3g} u, bound {n + 4} u"
    if c.family.startswith("split"):
        own = ec.split_owner(n, c.family == "split_end")
        for j in range(k):
            first, m = own[j]
            assert ec.outside_block_max(Z64[:, j], first, m) == 0.0, f"{what}: vector {j} is not zero outside rows [{first}, {first + m})"
            if m == 1:
                assert abs(Z64[first, j]) == 1.0, (what, j, Z64[first, j])
    ref = np.linalg.eigvalsh(ec.tridiag_dense(d, e))[::-1][:k]
    return float(np.abs(lam64 - ref).max() / delta), r_res, r_nrm


def eigsel_group(group, cases, dt):
    worst = [0.0, 0.0, 0.0]
    for c in cases:
        what = f"{ec.ecase_id(c)} {ec.dt_name(dt)}"
        lam, Z = run_eigsel([ec.ecase_de(c, dt)], c.k, dt, what)
        worst = [max(a, b) for a, b in zip(worst, check_eigsel(c, dt, lam[0], Z[0], what))]
    print(f"ratio[{group}] lam vs fp64 LAPACK / delta {worst[0]:.3e} (printed only: no truth for fp64), residual {worst[1]:.3e}, norm {worst[2]:.3e}: "
          f"{len(cases)} cases {ec.dt_name(dt)}")


@DT
@pytest.mark.parametrize("fam", ec.FAMILIES)
def test_eigsel_sizes(dt, fam):
    """Every family at n in {2, 3, 5, 63, 64, 65, 129, 200} (k = min(n, 6): kp = 8, two dead groups), toeplitz and split also at
    n = 1024 (k = 12)."""
    eigsel_group("eigsel-sizes", [c for c in ec.SIZE_CASES if c.family == fam], dt)


@DT
@pytest.mark.parametrize("fam", ["toeplitz", "split"])
def test_eigsel_lane_groupings(dt, fam):
    """n = 129, k in {1 .. 64}: G = 64 / kp lanes per eigenvalue from 64 down to 1, with and without dead groups."""
    eigsel_group("eigsel-k", [c for c in ec.SWEEP_CASES if c.family == fam], dt)


@DT
def test_eigsel_whole_spectrum(dt):
    """k = n at n in {2, 3, 5, 64}, every family."""
    eigsel_group("eigsel-k=n", ec.FULL_CASES, dt)


@DT
def test_eigsel_scaled(dt):
    """toeplitz and split times 2^+-20 (fp32) / 2^+-200 (fp64): inside the admissible range of a solver that does not rescale."""
    eigsel_group("eigsel-scaled", ec.SCALED_CASES, dt)


@DT
def test_eigsel_mixed_batch(dt):
    """Three families in one launch: the per-item offsets into d, e, lam, Z and the scratch."""
    cases = ec.MIXED_BATCH
    lam, Z = run_eigsel([ec.ecase_de(c, dt) for c in cases], cases[0].k, dt, "mixed batch")
    worst = [0.0, 0.0, 0.0]
    for b, c in enumerate(cases):
        worst = [max(x, y) for x, y in zip(worst, check_eigsel(c, dt, lam[b], Z[b], f"mixed batch item {b} {ec.ecase_id(c)}"))]
        one = run_eigsel([ec.ecase_de(c, dt)], c.k, dt, "single")
        assert same_bits(lam[b], one[0][0]) and same_bits(Z[b], one[1][0]), f"item {b} differs from the same item alone"
    print(f"ratio[eigsel-batch] lam vs fp64 LAPACK / delta {worst[0]:.3e} (printed only), residual {worst[1]:.3e}, norm {worst[2]:.3e}")


@DT
def test_eigsel_wilkinson_collapse_is_reported(dt):
    """W129+: the two largest eigenvalues agree to rounding.  Eigenvalues and residuals hold (test_eigsel_sizes); the two vectors
    coincide, and _hip.eigh_topk has to report the collapse through rmin.  Well separated spectra next to it are not reported."""
    h = _hip()
    n, k = 129, 4
    mats = {f: torch.as_tensor(ec.tridiag_dense(*ec.family(f, n))).to(dt) for f in ("wilkinson", "graded", "toeplitz")}
    for f, m in mats.items():
        X, lam, rmin = h.eigh_topk(m[None].to(DEV), k)
        print(f"rmin[{f} n={n} k={k} {ec.dt_name(dt)}] {float(rmin[0]):.3e}")
        assert torch.isfinite(rmin).all()
        assert (float(rmin[0]) < 0.5) == (f == "wilkinson"), (f, float(rmin[0]))
        d, e = ec.family(f, n)
        assert ec.certify_all(d, e, lam[0].double().cpu().numpy(), ec.C_LAMBDA * unit(dt) * ec.gershgorin(d, e)[2]) == [], f


# ------------------------------------------------------------------ ttr_tridiag_back
@functools.lru_cache(maxsize=4)
def _random_set(n, dt):
    return ec.random_reflectors(n, n + 3, 2, dt)


def run_back(A, tau, Z0, dt, what=""):
    """ttr_tridiag_back on A [B, n, lda] (all of it copied, NaN included, strideA = n lda + 5), tau [B, n], Z0 [B, n, k]: X on the
    CPU.  The inputs must keep their bits."""
    h = _hip()
    code = h.dtype_code(dt)
    B, n, lda = A.shape
    k = Z0.shape[2]
    a = Padded((B, n, lda), dt, lda, n * lda + 5, NAN, DEV)
    a.view().copy_(A)
    t = Padded.of(tau[None], 0, 0, NAN, DEV)
    z = Padded((B, n, k), dt, k, n * k, SENTINEL, DEV)
    z.refill(Z0)
    before = (a.buf.clone(), t.buf.clone())
    call("ttr_tridiag_back", code, n, B, k, a.ptr(), lda, a.stride, t.ptr(), z.ptr())
    assert torch.equal(bits(before[0]), bits(a.buf)) and torch.equal(bits(before[1]), bits(t.buf)), what
    return fetch(z, what + " Z")


@DT
@pytest.mark.parametrize("n", ec.BACK_N)
def test_back_random_reflectors(dt, n):
    """Random reflectors (a fifth of them H = I), NaN wherever the kernel must not read, Z random and not orthonormal: against the
    fp64 application of the same reflectors, within 4 x the error of the plain working-precision application (floor 8 u)."""
    A, tau = _random_set(n, dt)
    u, worst = unit(dt), 0.0
    for k in ec.back_ks(n):
        what = f"back n={n} k={k} {ec.dt_name(dt)}"
        g = torch.Generator().manual_seed(100 * n + k)
        Z0 = (3.0 * torch.randn(2, n, k, dtype=torch.float64, generator=g)).to(dt)
        X = run_back(A, tau, Z0, dt, what)
        for b in range(2):
            Ab, tb, Zb = A[b].numpy(), tau[b].numpy(), Z0[b].numpy()
            truth = ec.back_truth(Ab, tb, Zb)
            ref = ec.back_errors(Ab, tb, Zb, ec.back_ref(Ab, tb, Zb, dt), truth)
            err = ec.back_errors(Ab, tb, Zb, X[b].numpy(), truth)
            bound = ec.bound_u(ref / u) * u
            worst = max(worst, err / bound)
            assert err <= bound, f"{what} item {b}: {err / u:.3g} u max|Z|, the reference makes {ref / u:.3g} u, bound {bound / u:.3g} u"
    report("back", f"n={n} {ec.dt_name(dt)}", worst)


@DT
@pytest.mark.parametrize("n", ec.EXACT_N)
def test_back_exact_reflectors(dt, n):
    """Signed-permutation reflectors on integer Z: the fp64 result, value for value -- a wrong reflector index or order cannot hide."""
    A, tau = ec.exact_reflectors(n, n + 3, 2, dt)
    for k in ec.EXACT_K:
        g = torch.Generator().manual_seed(n + k)
        Z0 = torch.randint(-9, 10, (2, n, k), generator=g).to(dt)
        X = run_back(A, tau, Z0, dt, f"exact back n={n} k={k}")
        for b in range(2):
            truth = ec.back_truth(A[b].numpy(), tau[b].numpy(), Z0[b].numpy())
            gc.assert_exact(X[b], torch.as_tensor(truth.astype(np.float64)), f"exact back n={n} k={k} {ec.dt_name(dt)} item {b}")


@DT
def test_pipeline_tridiag_eigh_back(dt):
    """ttr_tridiag -> fp64 eigh of T on the host (exact Z, rounded to the dtype) -> ttr_tridiag_back at n = 129, lda = n + 3:
    ||A X - X Lambda||_F within the sum of the two stage bounds (eigsel_cases.pipeline_bound)."""
    n, k, b, u = 129, 6, 0, unit(dt)
    A0 = ec.tridiag_operand(n, b, dt)
    A_out, d, e, tau, _ = run_tridiag([A0], dt, ws=True, what="pipeline")
    w, V = np.linalg.eigh(ec.tridiag_dense(d[0].double().numpy(), e[0].double().numpy()))
    lam, Z = w[::-1][:k].copy(), torch.as_tensor(V[:, ::-1][:, :k].copy()).to(dt)
    Arefl = torch.full((1, n, n + 3), NAN, dtype=dt)
    Arefl[0, :, :n] = A_out[0]
    for r in range(n):
        Arefl[0, r, :r + 1] = NAN                     # what the back-transformation must not read
    X = run_back(Arefl, tau, Z[None], dt, "pipeline")[0].double().numpy()
    Zn, tn = Z.numpy(), tau[0].numpy()
    truth = ec.back_truth(Arefl[0].numpy(), tn, Zn)
    ref = ec.back_errors(Arefl[0].numpy(), tn, Zn, ec.back_ref(Arefl[0].numpy(), tn, Zn, dt), truth)
    A64 = A0.double().numpy()
    bound = ec.pipeline_bound(n, k, dt, ec.tridiag_bounds(dt, n, b)[0], ec.bound_u(ref / u) * u, np.abs(A64).max(),
                              np.linalg.norm(A64, 2), float(np.abs(Zn).max()))
    res = float(np.linalg.norm(A64 @ X - X * lam[None, :]))
    report("pipeline", f"n={n} k={k} {ec.dt_name(dt)}: ||A X - X Lambda||_F = {res:.3e}", res / bound)
    assert res <= bound

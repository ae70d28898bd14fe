"""TT completion (tn.als_completion) on the CPU: replay of the reference's fixture, an explicit Khatri-Rao ALS oracle, recovery of
an exact low-rank tensor, minimum-norm slices, the printed eps, and the error / x0 contract.  Also the device plan (AlsPlan: tasks
and chunks) on a CPU device and the argument envelope of the three completion entries of the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import tntorch_amd as tn
from tntorch_amd import _hip, _hipops, _hostops

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "completion_f64.npz")

# The documented shape rules of csrc/ttr_complete.hip, restated so that tests can bracket them
MAX_K = 1024  # r0 * r1 limit of all three entries
STAGE_BYTES = 48 * 1024  # LDS of ttr_als_normal's staged sample rows
SOLVE_LDS_BYTES = 60 * 1024  # ttr_spd_solve keeps (K * K + K) elements in LDS up to this size, global memory above


def elem_size(dtype):
    return torch.empty((), dtype=dtype).element_size()


def stage_rows(r0, r1, dtype):
    """Samples ttr_als_normal stages per pass: min(256, 48 KiB / ((r0 + r1 + 1) elem + 8)), rounded down to a multiple of 4."""
    return min(256, STAGE_BYTES // ((r0 + r1 + 1) * elem_size(dtype) + 8)) & ~3


def solve_lds_max_k(dtype):
    """The largest K whose system ttr_spd_solve factors in LDS; K + 1 runs in global memory."""
    K = 1
    while ((K + 1) * (K + 1) + (K + 1)) * elem_size(dtype) <= SOLVE_LDS_BYTES:
        K += 1
    return K


@pytest.fixture(autouse=True)
def _f64_default():
    """The fixture was recorded with float64 as the default dtype (x0 = None draws in it)."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


def fixture():
    return np.load(GOLDEN)


def case_args(z, name):
    """(X, y, ws, ranks_tt, niter, seed, x0 or None, init cores) of a replay case."""
    meta = [int(v) for v in z[name + "_meta"]]
    seed, niter, given = meta[:3]
    ranks = [r for r in meta[3:] if r]
    X, y = torch.from_numpy(z[name + "_X"]), torch.from_numpy(z[name + "_y"])
    ws = torch.from_numpy(z[name + "_ws"]) if name + "_ws" in z else None
    init = [torch.from_numpy(z["{}_init{}".format(name, n)]) for n in range(X.shape[1])]
    x0 = tn.Tensor([c.clone() for c in init]) if given else None
    return X, y, ws, ranks if len(ranks) > 1 else ranks[0], niter, seed, x0, init


def ref_train(z, name):
    return tn.Tensor([torch.from_numpy(z["{}_core{}".format(name, n)]) for n in range(z[name + "_X"].shape[1])])


def rel(a, b):
    return float((a - b).norm() / b.norm())


def values(t, X):
    return t[X].torch()


def oracle_als(X, y, w, cores, niter):
    """ALS on the explicit Khatri-Rao design matrices (columns (a, b) -> a r1 + b), lstsq(gelsd) per slice, QR gauges."""
    cores = [c.clone() for c in cores]
    N, P = len(cores), X.shape[0]

    def chain(cs, idx, left):
        v = torch.ones(P, 1, dtype=y.dtype)
        for c, i in (zip(cs, idx) if left else zip(reversed(cs), reversed(idx))):
            v = torch.einsum("pa,apb->pb", v, c[:, i, :]) if left else torch.einsum("apb,pb->pa", c[:, i, :], v)
        return v

    def solve(mu):
        Lp = chain(cores[:mu], [X[:, n] for n in range(mu)], True)
        Rp = chain(cores[mu + 1 :], [X[:, n] for n in range(mu + 1, N)], False)
        A = (Lp[:, :, None] * Rp[:, None, :]).reshape(P, -1) * w[:, None]
        new = torch.empty(Lp.shape[1], cores[mu].shape[1], Rp.shape[1], dtype=y.dtype)
        for i in range(new.shape[1]):
            sel = X[:, mu] == i
            new[:, i, :] = torch.linalg.lstsq(A[sel], (w * y)[sel, None], driver="gelsd").solution.reshape(new[:, i, :].shape)
        cores[mu] = new

    def orth(mu, left):
        c = cores[mu]
        if left:
            Q, R = torch.linalg.qr(c.reshape(-1, c.shape[2]))
            cores[mu], cores[mu + 1] = Q.reshape(c.shape[0], c.shape[1], -1), torch.einsum("ab,bic->aic", R, cores[mu + 1])
        else:
            Q, R = torch.linalg.qr(c.reshape(c.shape[0], -1).T)
            cores[mu], cores[mu - 1] = Q.T.reshape(-1, c.shape[1], c.shape[2]), torch.einsum("aib,cb->aic", cores[mu - 1], R)

    for n in range(N - 1, 0, -1):
        orth(n, False)
    for _ in range(niter):
        for mu in range(N - 1):
            solve(mu)
            orth(mu, True)
        for mu in range(N - 1, 0, -1):
            solve(mu)
            orth(mu, False)
    return tn.Tensor(cores)


def oracle_case(kind):
    """4- and 5-mode cases whose interior ranks exceed 1 (where the reference's reshape is wrong): X, y, w, x0 cores, niter."""
    shape, ranks, P, seed = {"n4": ([5, 6, 5, 6], [2, 3, 2], 900, 1), "n5": ([4, 5, 4, 5, 4], [2, 3, 3, 2], 1500, 2)}[kind]
    g = torch.Generator().manual_seed(seed)
    rs = [1] + ranks + [1]
    target = tn.Tensor([torch.randn(rs[n], shape[n], rs[n + 1], generator=g, dtype=torch.float64) for n in range(len(shape))])
    X = torch.stack([torch.randint(0, s, (P,), generator=g) for s in shape], dim=1)
    y = target[X].torch() + 1e-2 * torch.randn(P, generator=g, dtype=torch.float64)
    w = 0.5 + torch.rand(P, generator=g, dtype=torch.float64)
    x0 = [torch.rand(rs[n], shape[n], rs[n + 1], generator=g, dtype=torch.float64) for n in range(len(shape))]
    return X, y, w, x0, 3


@pytest.mark.parametrize("name", ["n2", "n2w", "n3x0", "n3"])
def test_golden_replay(name):
    z = fixture()
    X, y, ws, ranks, niter, seed, x0, init = case_args(z, name)
    torch.manual_seed(seed)
    if x0 is None:  # the seeded draw reproduces the reference's initial cores exactly
        drawn = tn.rand(list(init[n].shape[1] for n in range(len(init))), ranks_tt=ranks, dtype=torch.float64)
        assert all(torch.equal(a, b) for a, b in zip(drawn.cores, init))
        torch.manual_seed(seed)
    t = tn.als_completion(X, y, ranks_tt=ranks, ws=ws, x0=x0, niter=niter, verbose=False)
    ref = ref_train(z, name)
    assert rel(values(t, X), torch.from_numpy(z[name + "_values"])) < 1e-9
    assert rel(t.torch(), ref.torch()) < 1e-9


@pytest.mark.parametrize("kind", ["n4", "n5"])
def test_mirror_matches_khatri_rao_oracle(kind):
    X, y, w, x0, niter = oracle_case(kind)
    t = tn.als_completion(X, y, ranks_tt=None, ws=w, x0=tn.Tensor([c.clone() for c in x0]), niter=niter, verbose=False)
    o = oracle_als(X, y, w, x0, niter)
    assert rel(values(t, X), values(o, X)) < 1e-9
    assert rel(t.torch(), o.torch()) < 1e-9


def recovery_data(z):
    target = tn.Tensor([torch.from_numpy(z["rec4_target{}".format(n)]) for n in range(4)])
    X, Xh = torch.from_numpy(z["rec4_X"]), torch.from_numpy(z["rec4_Xh"])
    return target, X, Xh


def test_recovers_exact_rank3_where_reference_does_not():
    z = fixture()
    target, X, Xh = recovery_data(z)
    y, yh = target[X].torch(), target[Xh].torch()
    torch.manual_seed(int(z["rec4_seed"]))
    t = tn.als_completion(X, y, ranks_tt=3, niter=int(z["rec4_niter"]), verbose=False)
    assert rel(values(t, X), y) <= 1e-6 and rel(values(t, Xh), yh) <= 1e-6
    assert min(z["rec4_ref_err"]) > 5e-2  # the reference, same data and sweeps: its scrambled cores do not fit


def test_one_sample_per_slice():
    torch.manual_seed(0)
    I = 8
    X = torch.arange(I)[:, None].repeat(1, 2)
    y = torch.ones(I, dtype=torch.float64)
    t = tn.als_completion(X, y, ranks_tt=3, x0=tn.rand([I, I], ranks_tt=3, dtype=torch.float64), verbose=False)
    assert rel(values(t, X), y) < 1e-5


def test_rank_deficient_slice_is_minimum_norm():
    g = torch.Generator().manual_seed(3)
    P, r0, r1 = 20, 2, 3
    L, R = torch.randn(P, r0, generator=g, dtype=torch.float64), torch.randn(P, r1, generator=g, dtype=torch.float64)
    w, y = 0.5 + torch.rand(P, generator=g, dtype=torch.float64), torch.randn(P, generator=g, dtype=torch.float64)
    x = torch.cat([torch.zeros(2, dtype=torch.int64), torch.ones(P - 2, dtype=torch.int64)])  # slice 0: 2 samples < K = 6
    order = torch.argsort(x, stable=True)
    core = _hostops.als_core(L, R, w, y, order, [0, 2, P], 2)
    A = (L[:2, :, None] * R[:2, None, :]).reshape(2, -1) * w[:2, None]
    U, S, Vh = torch.linalg.svd(A, full_matrices=False)
    xmin = Vh.T @ ((U.T @ (w[:2] * y[:2])) / S)
    assert torch.allclose(core[:, 0, :].reshape(-1), xmin, rtol=0, atol=1e-12 * float(xmin.norm()))
    A1 = (L[2:, :, None] * R[2:, None, :]).reshape(P - 2, -1) * w[2:, None]
    full = torch.linalg.lstsq(A1, (w[2:] * y[2:])[:, None]).solution[:, 0]
    assert torch.allclose(core[:, 1, :].reshape(-1), full, rtol=0, atol=1e-12 * float(full.norm()))


def test_verbose_eps(capsys):
    z = fixture()
    X, y, ws, ranks, niter, seed, x0, init = case_args(z, "n2w")
    torch.manual_seed(seed)
    t = tn.als_completion(X, y, ranks_tt=ranks, ws=ws, niter=6, verbose=True)
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "Completing a 2D tensor of size [10, 12] using 300 samples..."
    eps = [float(m) for m in re.findall(r"\| eps: ([0-9.e+-]+) \| time:", "\n".join(out))]
    assert len(eps) == 6 and all(b <= a for a, b in zip(eps, eps[1:]))
    last = float((ws * (y - values(t, X))).norm() / y.norm())
    assert "{:.3e}".format(last) == "{:.3e}".format(eps[-1])


def test_errors_and_x0_contract():
    X = torch.tensor([[0, 0], [1, 1], [2, 0], [0, 2]])
    y = torch.ones(4, dtype=torch.float64)
    with pytest.raises(ValueError, match="One groundtruth sample is needed for every tensor slice"):
        tn.als_completion(X, y, ranks_tt=1, shape=[3, 4], verbose=False)
    with pytest.raises(AssertionError):
        tn.als_completion(X.double(), y, ranks_tt=1, verbose=False)
    with pytest.raises(ValueError, match="negative"):
        tn.als_completion(torch.tensor([[0, 0], [-1, 1], [1, 2]]), torch.ones(3, dtype=torch.float64), ranks_tt=1, verbose=False)
    torch.manual_seed(0)
    x0 = tn.rand([3, 3], ranks_tt=2, dtype=torch.float64)
    before = [c.clone() for c in x0.cores]
    storage = list(x0.cores)
    t = tn.als_completion(X, y, ranks_tt=5, x0=x0, niter=2, verbose=False)
    assert t is x0 and list(t.ranks_tt) == [1, 2, 1]  # ranks_tt ignored: x0's ranks
    assert all(torch.equal(a, b) for a, b in zip(storage, before))  # the caller's core storage is never written
    Xi = torch.tensor([[0, 0], [1, 1], [2, 2]], dtype=torch.int32)
    t = tn.als_completion(Xi, torch.ones(3, dtype=torch.float64), ranks_tt=1, verbose=False)
    assert list(t.shape) == [3, 3]


# ------------------------------------------------------------------------------------------------------------ device plan
@pytest.mark.parametrize("K", [1, 6, 96])
@pytest.mark.parametrize("budget", [1, 40 * 96 * 96 * 8, 1 << 40])
def test_als_plan_tasks_and_chunks(K, budget, monkeypatch):
    """Tasks partition every slice's samples in order (an empty slice: one empty task), none longer than max(ALS_TASK_SAMPLES,
    16 K); the chunks partition the slices, each within the byte budget of its systems or a single slice."""
    monkeypatch.setattr(_hipops, "ALS_TASK_SAMPLES", 40)
    monkeypatch.setattr(_hipops, "ALS_WORKSPACE_BYTES", budget)
    ts = max(40, 16 * K)
    counts = [0, 1, ts, ts + 1, 0, 3 * ts + 5, 7, ts - 1, 2 * ts, 0]
    elem = 8
    plan = _hipops.AlsPlan(counts, K, elem, torch.device("cpu"))
    tb, te, toff = plan.tb.tolist(), plan.te.tolist(), plan.toff.tolist()
    assert plan.counts.tolist() == counts
    assert len(toff) == len(counts) + 1 and toff[0] == 0 and len(tb) == len(te) == toff[-1]
    pos = 0
    for i, n in enumerate(counts):
        t0, t1 = toff[i], toff[i + 1]
        assert t1 - t0 == max(1, -(-n // ts)), (i, n)
        assert tb[t0] == pos and te[t1 - 1] == pos + n, (i, n)
        for t in range(t0, t1):
            assert 0 <= te[t] - tb[t] <= ts and (n == 0 or te[t] > tb[t]), (i, t)
            assert t == t0 or tb[t] == te[t - 1], (i, t)
        pos += n
    nxt = 0
    for i0, i1, t0, t1 in plan.chunks:
        assert i0 == nxt and i1 > i0 and (t0, t1) == (toff[i0], toff[i1])
        assert ((t1 - t0) + 3 * (i1 - i0)) * K * K * elem <= budget or i1 - i0 == 1, (i0, i1)
        nxt = i1
    assert nxt == len(counts)
    if budget == 1:
        assert len(plan.chunks) == len(counts)
    if budget == 1 << 40:
        assert len(plan.chunks) == 1


# ------------------------------------------------------------------------------------------------------------ C-ABI envelope
@pytest.fixture(scope="module")
def cabi():
    """The cross-compiled library, loaded without a device: every call below returns from its argument checks."""
    import __graft_entry__ as g

    g.build()
    L = ctypes.CDLL(g.LIB)
    for name in ("ttr_als_normal", "ttr_spd_solve", "ttr_pinv_finish"):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = _hip._SIGNATURES[name]
    L.ttr_last_error.restype = ctypes.c_char_p
    return L


def abi_code(name):
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ttround_hip.h")).read()
    return int(re.search(r"#define\s+" + name + r"\s+\(?(-?\d+)\)?", src).group(1))


def test_completion_entries_argument_envelope(cabi):
    OK, INVALID, UNSUPPORTED = abi_code("TTR_OK"), abi_code("TTR_E_INVALID"), abi_code("TTR_E_UNSUPPORTED")
    nul = [None] * 8

    def normal(dt, ntasks, r0, r1, ldl, ldr):
        return cabi.ttr_als_normal(dt, ntasks, r0, r1, None, ldl, None, ldr, *nul)

    def solve(dt, n, K):
        return cabi.ttr_spd_solve(dt, n, K, None, None, None, 0, None, 1, K, 1, 1, None, None, None, None, None)

    def finish(dt, n, K):
        return cabi.ttr_pinv_finish(dt, n, K, None, None, None, None, None, 1, K, 1, 1, None)

    for dt in (_hip.F32, _hip.F64):
        for r0, r1 in ((1, MAX_K + 1), (MAX_K + 1, 1), (32, 33)):
            assert normal(dt, 1, r0, r1, r0, r1) == UNSUPPORTED, (dt, r0, r1)
        assert b"above" in cabi.ttr_last_error()
        assert solve(dt, 1, MAX_K + 1) == UNSUPPORTED and solve(dt, 0, MAX_K + 1) == UNSUPPORTED
        assert finish(dt, 1, MAX_K + 1) == UNSUPPORTED and finish(dt, 0, MAX_K + 1) == UNSUPPORTED
        # K = 1024 passes the size checks and stops at the NULL pointers (no HIP call either way)
        assert normal(dt, 1, 1, MAX_K, 1, MAX_K) == INVALID and b"NULL" in cabi.ttr_last_error()
        assert solve(dt, 1, MAX_K) == INVALID and b"NULL" in cabi.ttr_last_error()
        assert finish(dt, 1, MAX_K) == INVALID and b"NULL" in cabi.ttr_last_error()
        assert normal(dt, 1, 4, 3, 3, 3) == INVALID and normal(dt, 1, 4, 3, 4, 2) == INVALID and normal(dt, -1, 4, 3, 4, 3) == INVALID
        assert normal(dt, 0, 4, 3, 4, 3) == OK and normal(dt, 0, 1, MAX_K, 1, MAX_K) == OK
        assert solve(dt, 0, 16) == OK and solve(dt, 0, MAX_K) == OK
        assert finish(dt, 0, 16) == OK and finish(dt, 0, MAX_K) == OK
    assert normal(2, 0, 4, 3, 4, 3) == INVALID and solve(2, 0, 16) == INVALID and finish(2, 0, 16) == INVALID

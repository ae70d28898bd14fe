"""TT completion on the MI355X: ttr_als_normal against an fp64 product of the explicit design matrix, ttr_spd_solve and its
minimum-norm fallback against LAPACK, device tn.als_completion against the CPU mirror, its envelope and its host reads."""
import pytest
import torch

import tntorch_amd as tn
from tntorch_amd import _hipops
from test_completion_host import (_f64_default, case_args, fixture, oracle_case, recovery_data, rel, solve_lds_max_k,  # noqa: F401
                                  values)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def normal_ref(L, R, w, y, x, I):
    A = (L.double()[:, :, None] * R.double()[:, None, :]).reshape(L.shape[0], -1)
    wd = w.double() if w is not None else torch.ones(L.shape[0], dtype=torch.float64)
    G = torch.stack([torch.einsum("pk,pl->kl", A[x == i] * wd[x == i, None] ** 2, A[x == i]) for i in range(I)])
    h = torch.stack([torch.einsum("pk,p->k", A[x == i], (wd ** 2 * y.double())[x == i]) for i in range(I)])
    return G, h


def run_normal(L, R, w, y, x, I):
    counts = torch.bincount(x, minlength=I).tolist()
    plan = _hipops.AlsPlan(counts, L.shape[1] * R.shape[1], L.element_size(), DEV)
    perm = torch.sort(x.to(DEV), stable=True).indices
    G, h = _hipops.als_normal(L.to(DEV), R.to(DEV), w.to(DEV) if w is not None else None, y.to(DEV), perm, plan)
    return G.cpu().double(), h.cpu().double(), plan


def check_normal(r0, r1, dtype, weighted, P=3000, I=5, x=None, seed=0):
    g = torch.Generator().manual_seed(seed)
    L, R = torch.randn(P, r0, generator=g).to(dtype), torch.randn(P, r1, generator=g).to(dtype)
    y = torch.randn(P, generator=g).to(dtype)
    w = (0.5 + torch.rand(P, generator=g)).to(dtype) if weighted else None
    x = torch.randint(0, I, (P,), generator=g) if x is None else x
    G, h, plan = run_normal(L, R, w, y, x, I)
    Gr, hr = normal_ref(L, R, w, y, x, I)
    tol = 1e-12 if dtype == torch.float64 else 2e-5
    assert float((G - Gr).abs().max()) <= tol * max(float(Gr.abs().max()), 1.0)
    assert float((h - hr).abs().max()) <= tol * max(float(hr.abs().max()), 1.0)
    return plan


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("r0,r1", [(1, 1), (1, 7), (5, 1), (3, 5), (8, 8), (7, 13), (16, 16), (32, 32), (1, 1024), (1024, 1),
                                   (64, 16), (16, 64), (31, 33), (2, 512), (1, 16), (1, 17), (17, 1), (4, 4)])
@pytest.mark.parametrize("weighted", [False, True])
def test_als_normal_matches_explicit_design(r0, r1, dtype, weighted):
    check_normal(r0, r1, dtype, weighted, P=2000 if r0 * r1 > 256 else 3000, I=3 if r0 * r1 > 256 else 5)


def test_als_normal_empty_segment():
    g = torch.Generator().manual_seed(1)
    x = torch.randint(0, 6, (1500,), generator=g)
    x[x == 2] = 3
    check_normal(4, 3, torch.float64, True, P=1500, I=6, x=x)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_als_normal_skewed_slice(dtype):
    P = 1 << 18
    g = torch.Generator().manual_seed(2)
    x = torch.where(torch.rand(P, generator=g) < 0.92, torch.zeros(P, dtype=torch.int64), torch.randint(1, 16, (P,), generator=g))
    plan = check_normal(4, 4, dtype, True, P=P, I=16, x=x)
    assert int(plan.toff[1]) >= 64  # the big slice is spread over many workgroups


def test_als_normal_chunks(monkeypatch):
    monkeypatch.setattr(_hipops, "ALS_WORKSPACE_BYTES", 12 * 64 * 64 * 8)  # two slices (2 tasks each) per chunk
    plan = check_normal(8, 8, torch.float64, True, P=20000, I=12)
    assert len(plan.chunks) >= 3


def spd_case(K, n_items, seed, deficient):
    """Partials of n_items systems: item i is A_i^T A_i (2 partials); deficient items get fewer rows than K."""
    g = torch.Generator().manual_seed(seed)
    As, Gs, hs, bs, counts = [], [], [], [], []
    for i in range(n_items):
        rows = K // 2 if i in deficient else K + 8
        A = torch.randn(rows, K, generator=g, dtype=torch.float64)
        b = torch.randn(rows, generator=g, dtype=torch.float64)
        h1 = rows // 2
        for sl in (slice(0, h1), slice(h1, rows)):
            Gs.append(A[sl].T @ A[sl])
            hs.append(A[sl].T @ b[sl])
        As.append(A)
        bs.append(b)
        counts.append(rows)
    return As, bs, torch.stack(Gs), torch.stack(hs), torch.tensor(counts)


@pytest.mark.parametrize("dtype,K", [(dt, K) for dt in (torch.float64, torch.float32)
                                     for K in (6, 64, 100, solve_lds_max_k(dt), solve_lds_max_k(dt) + 1)])
def test_spd_solve_and_minimum_norm_fallback(dtype, K):
    """fp32 partials (rounded from the fp64 ones): Cholesky within K eps cond(G), the minimum-norm items within K eps cond_r (the
    retained spectrum) of the fp64 references (C = 1; the measured constants are in test_completion_kernels_gpu)."""
    n = 7
    deficient = {1, 4}
    As, bs, Gp, hp, counts = spd_case(K, n, K, deficient)
    Gp, hp = Gp.to(dtype), hp.to(dtype)
    X = torch.full((n, 1, K), float("nan"), dtype=dtype, device=DEV)
    status = _hipops.spd_solve_batch(Gp.to(DEV), hp.to(DEV), torch.arange(0, 2 * n + 1, 2, device=DEV), X, K,
                                     counts=counts.to(DEV))
    st, X = status.cpu().tolist(), X.cpu()[:, 0, :].double()
    eps32 = 2.0 ** -23
    for i in range(n):
        G, h = Gp[2 * i].double() + Gp[2 * i + 1].double(), hp[2 * i].double() + hp[2 * i + 1].double()
        if i in deficient:
            assert st[i] == 0
            ref = torch.linalg.lstsq(As[i], bs[i][:, None], driver="gelsd").solution[:, 0]
            sv = torch.linalg.svdvals(As[i])
            tol = 1e-8 if dtype == torch.float64 else K * eps32 * float(sv[0] / sv[-1]) ** 2
            assert float((X[i] - ref).norm()) <= tol * float(ref.norm())
        else:
            assert st[i] == 1
            ref = torch.linalg.solve(G, h)
            lam = torch.linalg.eigvalsh(G)
            tol = 1e-9 if dtype == torch.float64 else K * eps32 * float(lam[-1] / lam[0])
            assert float((X[i] - ref).norm()) <= tol * float(ref.norm())


def test_spd_solve_flags_degenerate_design_by_pivot():
    K, n = 16, 3
    g = torch.Generator().manual_seed(9)
    Gp, hp, As, bs = [], [], [], []
    for i in range(n):
        A = torch.randn(40, K, generator=g, dtype=torch.float64)
        if i == 1:  # rank K - 3 with 40 >= K samples: only the pivots reveal it
            A = torch.randn(40, K - 3, generator=g, dtype=torch.float64) @ torch.randn(K - 3, K, generator=g, dtype=torch.float64)
        b = torch.randn(40, generator=g, dtype=torch.float64)
        Gp.append(A.T @ A)
        hp.append(A.T @ b)
        As.append(A)
        bs.append(b)
    X = torch.zeros((n, 1, K), dtype=torch.float64, device=DEV)
    status = _hipops.spd_solve_batch(torch.stack(Gp).to(DEV), torch.stack(hp).to(DEV), torch.arange(n + 1, device=DEV), X, K)
    assert status.cpu().tolist() == [1, 0, 1]
    ref = torch.linalg.lstsq(As[1], bs[1][:, None], driver="gelsd").solution[:, 0]
    assert float((X.cpu()[1, 0] - ref).norm()) <= 1e-8 * float(ref.norm())


def dev_tensor(cores, dtype=torch.float64):
    return tn.Tensor([c.to(DEV, dtype) for c in cores])


@pytest.mark.parametrize("name", ["n2", "n2w", "n3x0", "n3"])
def test_device_matches_mirror_on_golden(name):
    z = fixture()
    X, y, ws, ranks, niter, seed, x0, init = case_args(z, name)
    torch.manual_seed(seed)
    host = tn.als_completion(X, y, ranks_tt=ranks, ws=ws, x0=x0, niter=niter, verbose=False)
    torch.manual_seed(seed)
    x0d = dev_tensor(init) if x0 is not None else None
    dev = tn.als_completion(X.to(DEV), y.to(DEV), ranks_tt=ranks, ws=ws.to(DEV) if ws is not None else None, x0=x0d, niter=niter,
                            verbose=False)
    assert dev.cores[0].is_cuda
    dcpu = tn.Tensor([c.cpu() for c in dev.cores])
    assert rel(values(dcpu, X), values(host, X)) < 1e-8
    assert rel(dcpu.torch(), host.torch()) < 1e-8


@pytest.mark.parametrize("kind", ["n4", "n5"])
def test_device_matches_mirror_on_oracle_cases(kind):
    X, y, w, x0, niter = oracle_case(kind)
    host = tn.als_completion(X, y, ranks_tt=None, ws=w, x0=tn.Tensor([c.clone() for c in x0]), niter=niter, verbose=False)
    dev = tn.als_completion(X.to(DEV), y.to(DEV), ranks_tt=None, ws=w.to(DEV), x0=dev_tensor(x0), niter=niter, verbose=False)
    dcpu = tn.Tensor([c.cpu() for c in dev.cores])
    assert rel(values(dcpu, X), values(host, X)) < 1e-8


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-6), (torch.float32, 1e-3)])
def test_device_recovery(dtype, tol):
    z = fixture()
    target, X, Xh = recovery_data(z)
    y, yh = target[X].torch(), target[Xh].torch()
    torch.manual_seed(int(z["rec4_seed"]))
    x0 = dev_tensor(tn.rand([10] * 4, ranks_tt=3).cores, dtype)
    t = tn.als_completion(X.to(DEV), y.to(DEV, dtype), ranks_tt=3, x0=x0, niter=int(z["rec4_niter"]) + 5, verbose=False)
    tc = tn.Tensor([c.cpu().double() for c in t.cores])
    assert rel(values(tc, X), y) <= tol and rel(values(tc, Xh), yh) <= tol


def test_device_avoids_torch_linalg(monkeypatch):
    def banned(*a, **k):
        raise AssertionError("torch linear algebra reached by device completion")

    X, y, w, x0, niter = oracle_case("n4")
    Xd, yd, wd, x0d = X.to(DEV), y.to(DEV), w.to(DEV), dev_tensor(x0)
    for name in ("einsum", "matmul", "bmm", "mm"):
        monkeypatch.setattr(torch, name, banned)
    monkeypatch.setattr(torch.Tensor, "__matmul__", banned)
    for name in ("qr", "lstsq", "solve", "inv", "lu_factor", "svd", "eigh", "pinv", "norm", "vector_norm", "solve_triangular",
                 "cholesky", "det"):
        monkeypatch.setattr(torch.linalg, name, banned)
    t = tn.als_completion(Xd, yd, ranks_tt=None, ws=wd, x0=x0d, niter=2, verbose=True)
    monkeypatch.undo()
    assert all(c.is_cuda for c in t.cores)


def test_no_host_reads_per_sweep(monkeypatch):
    X, y, w, x0, _ = oracle_case("n5")
    Xd, yd, wd = X.to(DEV), y.to(DEV), w.to(DEV)
    shape = [int(s) for s in (X.max(dim=0)[0] + 1)]

    def count(niter):
        x0d = dev_tensor(x0)
        torch.cuda.synchronize()
        n = [0]
        for cls, name in ((torch.Tensor, "item"), (torch.Tensor, "tolist"), (torch.Tensor, "cpu"), (torch.cuda, "synchronize")):
            orig = getattr(cls, name)

            def wrap(*a, _o=orig, **k):
                n[0] += 1
                return _o(*a, **k)

            monkeypatch.setattr(cls, name, wrap)
        tn.als_completion(Xd, yd, ranks_tt=None, shape=shape, ws=wd, x0=x0d, niter=niter, verbose=False)
        monkeypatch.undo()
        return n[0]

    assert count(1) == count(4)


def test_device_rank_limit():
    I = 40
    X = torch.arange(I)[:, None].repeat(1, 3).to(DEV)
    x0 = dev_tensor(tn.rand([I] * 3, ranks_tt=33, dtype=torch.float64).cores)
    with pytest.raises(NotImplementedError, match="1024"):
        tn.als_completion(X, torch.ones(I, dtype=torch.float64, device=DEV), ranks_tt=None, x0=x0, verbose=False)

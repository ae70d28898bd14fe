"""Drop-in API on CPU tensors (the host mirror): golden vectors + the reference's own
property tests (tests/test_round.py, tests/test_tensor.py, tests/test_init.py, tests/test_tools.py)."""
import numpy as np
import pytest
import torch

import oracle
import tntorch_amd as tn
from parity import analytic_128, load_case, load_meta


def _max_abs(a, b):
    return max((x - y).abs().max().item() for x, y in zip(a, b))


@pytest.fixture(autouse=True)
def _f64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


@pytest.mark.parametrize("alg", ["svd", "eig"])
def test_golden_round(alg):
    g = load_case("round_eps_f64")
    t = tn.round_tt(tn.Tensor(g["inp"]), eps=1e-8, algorithm=alg)
    assert t.ranks_tt.tolist() == [1, 4, 4, 4, 4, 4, 4, 4, 1]
    # up to the per-bond sign of the singular vectors, which LAPACK builds choose differently ('eig': MKL's code paths differ)
    assert _max_abs(oracle.gauge_align(g[alg], t.cores), g[alg]) < 1e-9
    g = load_case("round_batch_f64")
    t = tn.Tensor(g["inp"], batch=True)
    t.round_tt(rmax=2, algorithm=alg)
    assert _max_abs(t.cores, g[alg]) < 1e-10


@pytest.mark.parametrize("alg", ["svd", "eig"])
def test_golden_dense(alg):
    g = load_case("dense_f64")
    t = tn.Tensor(g["X"], ranks_tt=4, algorithm=alg)
    assert _max_abs(t.cores, g[alg]) < 1e-9
    g = load_case("dense_batch_f32")
    t = tn.Tensor(g["X"], ranks_tt=3, batch=True, algorithm=alg)
    ref = oracle.tt_to_dense(g[alg], batch=True)
    assert (t.torch() - ref).norm() / ref.norm() < 1e-4


def test_c0_config_cpu():
    """BASELINE config C0: tn.Tensor(torch.randn(16,16,16,16)).round_tt(rmax=4) on CPU PyTorch."""
    g = load_case("c0_16x4_rmax4_f32")
    torch.manual_seed(0)
    X = torch.randn(16, 16, 16, 16, dtype=torch.float32)
    t = tn.Tensor(X)
    assert [tuple(c.shape) for c in t.cores] == [(1, 16, 16), (16, 16, 256), (256, 16, 16), (16, 16, 1)]
    assert torch.equal(t.torch(), X)
    t.round_tt(rmax=4)
    assert t.ranks_tt.tolist() == [1, 4, 4, 4, 1]
    d, dref = t.torch(), oracle.tt_to_dense(g["svd"])
    assert (d - dref).norm() / dref.norm() < 1e-4
    assert abs((d - X).norm() / X.norm() - (dref - X).norm() / X.norm()) < 1e-5


def test_golden_truncated_svd_and_orthogonalize():
    g = load_case("truncated_svd_f64")
    for c in load_meta()["cases"]["truncated_svd_f64"]["calls"]:
        kw = {k: c[k] for k in ("eps", "rmax", "delta") if k in c}
        u, v = tn.truncated_svd(g["M_" + c["M"]], left_ortho=c["left_ortho"], algorithm=c["algorithm"], **kw)
        assert (u - g[f"call{c['i']}_left"]).abs().max() < 1e-10 and (v - g[f"call{c['i']}_right"]).abs().max() < 1e-10
    g = load_case("orthogonalize_f64")
    for name, fn in [("left0", lambda t: t.left_orthogonalize(0)), ("right4", lambda t: t.right_orthogonalize(4)),
                     ("orth2", lambda t: t.orthogonalize(2)), ("orth4", lambda t: t.orthogonalize(4))]:
        t = tn.Tensor([c.clone() for c in g["inp"]])
        fn(t)
        assert _max_abs(t.cores, g[name]) < 1e-12, name


def test_known_answers_notebook():
    full = analytic_128()
    t = tn.Tensor(full, ranks_tt=3)
    assert t.ranks_tt.tolist() == [1, 3, 3, 1]
    assert abs(tn.relative_error(full, t).item() - 5.122978e-4) < 1e-9
    t = tn.Tensor(full)
    t.round_tt(eps=1e-5)
    assert t.ranks_tt.tolist() == [1, 4, 6, 1]
    assert abs(tn.relative_error(full, t).item() - 8.3358e-06) < 1e-9


# ---- the reference's own tests, against this class --------------------------------------------
def test_ref_orthogonalization():  # tests/test_round.py:7-18
    np.random.seed(0)
    for _ in range(30):
        gt = tn.rand(np.random.randint(1, 8, np.random.randint(2, 6)), ranks_tt=np.random.randint(1, 5))
        t = gt.clone()
        assert tn.relative_error(gt, t) <= 1e-7
        t.left_orthogonalize(0)
        assert tn.relative_error(gt, t) <= 1e-7
        t.right_orthogonalize(t.dim() - 1)
        assert tn.relative_error(gt, t) <= 1e-7
        t.orthogonalize(np.random.randint(t.dim()))
        assert tn.relative_error(gt, t) <= 1e-7


@pytest.mark.parametrize("alg", ["svd", "eig"])
def test_ref_truncated_svd_batch_equals_loop(alg):  # tests/test_round.py:21-38
    gt = torch.rand((2, 32, 32))
    u, v = tn.truncated_svd(gt, batch=True, algorithm=alg)
    for i in range(len(gt)):
        u1, v1 = tn.truncated_svd(gt[i], batch=False, algorithm=alg)
        assert torch.allclose(u1 @ v1, u[i] @ v[i])


def test_ref_round_tt_svd_rank_recovery():  # tests/test_round.py:41-49
    np.random.seed(1)
    for _ in range(20):
        gt = tn.rand(np.random.randint(1, 8, np.random.randint(8, 10)), ranks_tt=np.random.randint(1, 10))
        gt.round_tt(1e-8, algorithm="svd")
        t = gt + gt
        t.round_tt(1e-8, algorithm="svd")
        assert tn.relative_error(gt, t / 2) <= 1e-4
        assert max(gt.ranks_tt) == max(t.ranks_tt)


def test_ref_tt_tensor_batch_equals_loop():  # tests/test_tensor.py:28-49
    torch.manual_seed(1)
    for shape in [(10, 5, 5, 5, 5), (4, 2, 2, 2, 2, 2, 2, 2, 2)]:
        a = torch.rand(*shape)
        b = tn.Tensor(a, ranks_tt=3, batch=True)
        for i in range(len(a)):
            c = tn.Tensor(a[i], ranks_tt=3, batch=False)
            for j, core in enumerate(c.cores):
                assert torch.allclose(core, b.cores[j][i, ...])
            assert torch.allclose(c.torch(), b.torch()[i])


def test_ref_round_tt_keeps_tensor():  # tests/test_tensor.py:361-392
    torch.manual_seed(2)
    t = tn.rand([8] * 4, ranks_tt=5)
    X = t.torch()
    t.round_tt(eps=1e-8)
    assert torch.norm(X - t.torch()) / torch.norm(X) < 1e-8
    tb = tn.rand([3, 8, 8, 8], ranks_tt=5, batch=True)
    Xb = tb.torch()
    tb.round_tt(eps=1e-8)
    assert torch.norm(Xb - tb.torch()) / torch.norm(Xb) < 1e-8


def test_ref_from_ndarray():  # tests/test_init.py:7-13
    np.random.seed(3)
    for _ in range(30):
        gt = np.random.rand(*np.random.randint(1, 8, np.random.randint(1, 6)))
        t = tn.Tensor(gt)
        assert np.linalg.norm(gt - t.numpy()) / np.linalg.norm(gt) <= 1e-7


def test_ref_unfolding():  # tests/test_tools.py:7-10
    X = torch.rand(3, 4, 5, 6)
    assert torch.equal(tn.unfolding(X, 2), X.permute(2, 0, 1, 3).reshape(5, -1))
    assert torch.equal(tn.unfolding(X, 1, batch=True), X.permute(0, 2, 1, 3).reshape(3, 5, -1))
    c = torch.rand(2, 3, 4)
    assert tn.left_unfolding(c).shape == (6, 4) and tn.right_unfolding(c).shape == (2, 12)
    assert tn.left_unfolding(X, batch=True).shape == (3, 20, 6) and tn.right_unfolding(X, batch=True).shape == (3, 4, 30)


def test_api_errors_and_quirks():
    M = torch.rand(4, 5)
    with pytest.raises(ValueError, match="either"):
        tn.truncated_svd(M, delta=0.1, eps=0.1)
    with pytest.raises(AssertionError):
        tn.truncated_svd(M, algorithm="qr")
    with pytest.raises(ValueError, match="ranks do not match"):
        tn.Tensor([torch.rand(1, 3, 2), torch.rand(3, 3, 1)])
    with pytest.raises(ValueError):
        tn.Tensor("nope")
    t = tn.rand([4, 4, 4], ranks_tt=2)
    with pytest.raises(AssertionError):
        t.round_tt(rmax=[1])
    with pytest.raises(AssertionError):
        t.left_orthogonalize(2)
    with pytest.raises(ValueError, match="CP-TT"):
        tn.Tensor(torch.rand(4, 4, 4), ranks_cp=2, ranks_tt=2)       # tensor.py:211-212
    # quirks 1, 5, 13, 14
    assert tn.Tensor(torch.ones(4, 4, 4), ranks_tt=3).ranks_tt.tolist() == [1, 1, 1, 1]
    z = tn.Tensor([torch.zeros(1, 5, 3), torch.zeros(3, 5, 3), torch.zeros(3, 5, 1)])
    z.round_tt()
    assert z.ranks_tt.tolist() == [1, 1, 1, 1]
    t = tn.rand([5, 5, 5, 5], ranks_tt=4)
    before = [c.clone() for c in t.cores]
    t2 = tn.round_tt(t, rmax=2)  # free function clones (round.py:17)
    assert _max_abs(t.cores, before) == 0 and t2.ranks_tt.tolist() == [1, 2, 2, 2, 1]
    t.ranks_tt = 3  # setter rounds in place (tensor.py:885-888)
    assert t.ranks_tt.tolist() == [1, 3, 3, 3, 1]
    # arithmetic used around the path
    a, b = tn.rand([3, 4, 5], ranks_tt=2), tn.rand([3, 4, 5], ranks_tt=3)
    assert torch.allclose((a + b).torch(), a.torch() + b.torch())
    assert torch.allclose((a - b).torch(), a.torch() - b.torch())
    assert torch.allclose((a * 2.5).torch(), a.torch() * 2.5) and torch.allclose((a / 2).torch(), a.torch() / 2)
    assert torch.allclose((a + 1.5).torch(), a.torch() + 1.5)
    assert abs(tn.dot(a, b).item() - (a.torch() * b.torch()).sum().item()) < 1e-9
    assert abs(tn.norm(a).item() - a.torch().norm().item()) < 1e-9


# ------------------------------------------------------------------ Tucker rounding / round() on the host mirror (8f-2)
def _tk(cores):
    return [c.shape[-2] for c in cores]


@pytest.mark.parametrize("alg", ["svd", "eig"])
def test_host_round_tucker_golden(alg):
    from parity import load_case
    g = load_case("round_tucker_eps_f64")
    t = tn.Tensor([c.clone() for c in g["inp"]])
    t.round_tucker(eps=1e-8, algorithm=alg)
    assert _tk(t.cores) == _tk(g[f"{alg}_cores"])
    assert max((a - b).abs().max().item() for a, b in zip(t.cores, g[f"{alg}_cores"])) < 1e-8
    assert max((a - b).abs().max().item() for a, b in zip(t.Us, g[f"{alg}_Us"])) < 1e-8
    assert tuple(t.shape) == (12, 10, 14, 11) and t.ranks_tucker.tolist() == _tk(t.cores)
    X = oracle.tt_to_dense(g["inp"])
    assert (t.torch() - X).norm() / X.norm() < 1e-8
    # batch mode
    gb = load_case("round_tucker_batch_f64")
    tb = tn.Tensor([c.clone() for c in gb["inp"]], batch=True)
    tb.round_tucker(rmax=2, algorithm=alg)
    assert max((a - b).abs().max().item() for a, b in zip(tb.cores, gb[f"{alg}_cores"])) < 1e-9
    assert max((a - b).abs().max().item() for a, b in zip(tb.Us, gb[f"{alg}_Us"])) < 1e-9


@pytest.mark.parametrize("alg", ["svd", "eig"])
def test_host_ctor_tucker_and_round_golden(alg):
    from parity import load_case
    g = load_case("ctor_tucker_f64")
    t = tn.Tensor(g["inp"], ranks_tucker=4, ranks_tt=3, algorithm=alg)
    assert t.ranks_tt.tolist() == [1, 3, 3, 3, 1] and t.ranks_tucker.tolist() == [4, 4, 4, 4]
    assert max((a - b).abs().max().item() for a, b in zip(t.cores, g[f"{alg}_cores"])) < 1e-8
    assert max((a - b).abs().max().item() for a, b in zip(t.Us, g[f"{alg}_Us"])) < 1e-8
    g = load_case("round_general_f64")
    t = tn.round(tn.Tensor([c.clone() for c in g["inp"]]), eps=1e-6, algorithm=alg)
    assert oracle.tt_ranks(t.cores) == oracle.tt_ranks(g[f"{alg}_cores"]) and _tk(t.cores) == _tk(g[f"{alg}_cores"])
    ref = oracle.tucker_to_dense(g[f"{alg}_cores"], g[f"{alg}_Us"])
    assert (t.torch() - ref).norm() / ref.norm() < 1e-9
    # factors survive +, scalar *, clone, dot
    u = t + t
    assert (u.torch() - 2 * ref).norm() / ref.norm() < 1e-9
    assert abs(tn.dot(t, t).item() - (ref * ref).sum().item()) < 1e-9 * (ref * ref).sum().item()
    assert ((t * 3).torch() - 3 * ref).norm() / ref.norm() < 1e-9


def test_host_known_answer_eps_ctor():
    """decompositions.ipynb cell 14: tn.Tensor(full, eps=1e-5)."""
    from parity import analytic_128
    full = analytic_128()
    t = tn.Tensor(full, eps=1e-5)
    assert t.ranks_tt.tolist() == [1, 4, 6, 1] and t.ranks_tucker.tolist() == [4, 5, 6]
    assert abs(tn.relative_error(full, t).item() - 8.340228167320888e-06) < 1e-9


# ------------------------------------------------------------------ CP-ALS on the host mirror (8f-1)
def test_host_cp_als_golden():
    from parity import load_case, load_meta
    g = load_case("cp_als")
    runs = load_meta()["cases"]["cp_als"]["runs"]
    for name in ("r3_it1", "r3_it25", "r5_it4"):
        t = tn.Tensor(g["inp"], ranks_cp=runs[name]["R"], max_iter=runs[name]["max_iter"])
        assert all(c.dim() == 2 for c in t.cores) and tuple(t.shape) == (12, 10, 9, 11)
        # (MKL's lstsq / eigh are not bit-reproducible from run to run, not even single-threaded: the factors of identical calls differ
        # by 0 ... 8e-11 here -- mostly exactly 0, the rank-5 case is the sensitive one -- and the reconstruction by up to 2e-13)
        assert max((a - b).abs().max().item() for a, b in zip(t.cores, g[name])) < 1e-7
        assert abs(tn.relative_error(g["inp"], t).item() - runs[name]["relerr"]) < 1e-12   # (observed: up to 2e-13)
    # CP factors behave as TT cores with diagonal slices everywhere else (tensor.py:1717-1769)
    ref = oracle.cp_to_dense(g["r5_it4"])
    assert (t.torch() - ref).norm() / ref.norm() < 2e-12   # (0 on most runs; 2.2e-13 seen once in ~30: a bound ~10x the observed noise)
    assert t.ranks_tt.tolist() == [5, 5, 5, 5, 5]
    u = t.clone()
    u.round_tt(eps=1e-10)
    assert u.ranks_tt.tolist() == [1, 5, 5, 5, 1] and (u.torch() - ref).norm() / ref.norm() < 1e-9
    with pytest.raises(ValueError):
        tn.Tensor(g["inp"], ranks_cp=3, ranks_tt=2)


# ------------------------------------------------------------------ producers on the host mirror (8f-3)
def test_host_producers_golden():
    import operator
    from parity import load_case, load_meta
    g = load_case("producers_f64")
    a, b = tn.Tensor(g["a"]), tn.Tensor(g["b"])
    p = a * b
    assert max((x - y).abs().max().item() for x, y in zip(p.cores, g["prod"])) == 0
    assert (p.torch() - a.torch() * b.torch()).abs().max() < 1e-12
    ts = [tn.Tensor(g[f"t{i}"]) for i in range(5)]
    red = tn.reduce(ts, operator.add, eps=1e-6)
    ref = g["red_dense"]
    assert red.ranks_tt.tolist() == g["red_ranks_tt"].tolist() and red.ranks_tucker.tolist() == g["red_ranks_tucker"].tolist()
    assert (red.torch() - ref).norm() / ref.norm() < 1e-9
    red3 = tn.reduce(ts, operator.add, rmax=3)
    ref3 = oracle.tt_to_dense(g["red3_cores"])
    assert (red3.torch() - ref3).norm() / ref3.norm() < 1e-10
    # docs/tutorials/arithmetics.ipynb cell 1
    ones = tn.ones([32] * 4)
    assert tn.round((ones + ones) * (ones - 2)).ranks_tt.tolist() == load_meta()["known_answers"]["measured_with_reference_here"]["arith_round_ranks"]


# ------------------------------------------------------------------ consumers on the host mirror (8f-4)
SHIFT_SPECS = [(1, 2, 1e-3), (3, -2, 1e-6), (0, 4, "same"), (4, -4, 1e-2), (2, 1, 0.3)]


def test_host_shift_mode_and_ttmatrix_golden():
    from parity import load_case
    g = load_case("consumers_f64")
    for k, (n, sh, eps) in enumerate(SHIFT_SPECS):
        t = tn.Tensor([c.clone() for c in g["g"]])
        r = tn.shift_mode(t, n, sh, eps=eps)
        assert r is t  # in place on the core list (tools.py:650-697)
        want = g[f"shift{k}"]
        assert [tuple(c.shape) for c in t.cores] == [tuple(c.shape) for c in want]
        assert max((a - b).abs().max().item() for a, b in zip(t.cores, want)) < 1e-10
    t = tn.Tensor([c.clone() for c in g["g"]])
    assert tn.shift_mode(t, 2, 0) is t
    with pytest.raises(ValueError):
        tn.shift_mode(t, 1, 1, eps=-1.0)
    with pytest.raises(AssertionError):
        tn.shift_mode(t, 3, 2)
    ttm = tn.TTMatrix(g["m"], input_dims=[11, 3, 4], output_dims=[23, 2, 3], ranks=[20, 7])
    assert ttm.ranks.tolist() == [20, 7] and not ttm.batch
    assert max((a - b).abs().max().item() for a, b in zip(ttm.cores, g["ttm_cores"])) < 1e-10
    assert (ttm.torch() - g["ttm_dense"]).abs().max() < 1e-12
    tsq = tn.TTMatrix(g["sq"], input_dims=[6, 5], output_dims=[6, 5], ranks=[36])
    assert abs(tsq.trace().item() - g["tsq_trace"].item()) < 1e-12
    again = tn.TTMatrix(ttm.cores, None, [11, 3, 4], [23, 2, 3])  # from pre-processed cores (matrix.py:48-57)
    assert again.ranks.tolist() == [20, 7] and (again.torch() - g["ttm_dense"]).abs().max() < 1e-12
    assert list(ttm.flatten().shape) == [11 * 23, 3 * 2, 4 * 3]


def test_host_ttmatrix_batch_matches_items():
    """The reference's batched TTMatrix constructor raises (matrix.py:73 builds a tensor from a list of tuples); here the
    batch path works and equals the per-item construction."""
    torch.manual_seed(5)
    mb = torch.rand(3, 6 * 5, 4 * 3, dtype=torch.float64)
    b = tn.TTMatrix(mb, input_dims=[6, 5], output_dims=[4, 3], ranks=[5])
    assert b.batch and [tuple(c.shape) for c in b.cores] == [(3, 1, 6, 4, 5), (3, 5, 5, 3, 1)]
    for k in range(3):
        one = tn.TTMatrix(mb[k], input_dims=[6, 5], output_dims=[4, 3], ranks=[5])
        assert (one.torch() - b.torch()[k]).abs().max() < 1e-12
    sq = torch.rand(2, 12, 12, dtype=torch.float64)
    tb = tn.TTMatrix(sq, input_dims=[4, 3], output_dims=[4, 3], ranks=[16])
    assert (tb.trace() - torch.stack([torch.trace(x) for x in sq])).abs().max() < 1e-11


def test_host_decompress_tucker_factors():
    torch.manual_seed(8)
    t = tn.rand([5, 6, 7], ranks_tt=3, ranks_tucker=[2, 3, 4], dtype=torch.float64)
    d = t.decompress_tucker_factors()
    assert all(U is None for U in d.Us) and (d.torch() - t.torch()).abs().max() < 1e-12
    d1 = t.decompress_tucker_factors(dim=1)
    assert d1.Us[0] is not None and d1.Us[1] is None and (d1.torch() - t.torch()).abs().max() < 1e-12
    moved = tn.shift_mode(tn.Tensor([c.clone() for c in t.cores], Us=[U.clone() for U in t.Us]), 0, 2, eps=1e-10)
    assert (moved.torch() - t.torch().permute(1, 2, 0)).abs().max() < 1e-8


def test_host_cp_variants_golden():
    """Batched CP-ALS and CP on a Tucker core on the host mirror = the reference's recorded outputs."""
    from parity import load_case
    g = load_case("cp_variants_f64")
    tb = tn.Tensor(g["batch_inp"], ranks_cp=4, batch=True, max_iter=6, tol=-1.0)
    assert tb.batch and [tuple(c.shape) for c in tb.cores] == [(3, 8, 4), (3, 7, 4), (3, 6, 4)] and len(tb.cp_errors) == 6
    assert max((a - b).abs().max().item() for a, b in zip(tb.cores, g["batch_r4_it6"])) < 1e-7
    assert (tb.torch() - g["batch_dense"]).abs().max() < 1e-7
    torch.manual_seed(21)
    tt = tn.Tensor(g["tucker_inp"], ranks_cp=3, ranks_tucker=4, max_iter=5, tol=-1.0)
    assert [tuple(c.shape) for c in tt.cores] == [(4, 3)] * 3 and [tuple(U.shape) for U in tt.Us] == [(9, 4), (8, 4), (7, 4)]
    assert (tt.torch() - g["tucker_dense"]).abs().max() < 1e-8
    with pytest.raises(ValueError):
        tn.Tensor(g["tucker_inp"], ranks_cp=3, ranks_tt=2)


def test_rand_tucker_only_gets_full_tt_ranks():
    """create.py:243-272: `ranks_tucker` without `ranks_tt` builds a TT-Tucker tensor whose core has full TT ranks (round-2
    advisor finding: this used to raise)."""
    for shape, rk, want in (([5, 6, 7, 4], 3, [1, 3, 9, 3, 1]), ([5, 6, 7, 4], [2, 3, 4, 2], [1, 2, 6, 2, 1]),
                            ([8, 8, 8], [None, 3, 2], [1, 6, 2, 1])):
        t = tn.rand(shape, ranks_tucker=rk)
        assert t.ranks_tt.tolist() == want and tuple(t.shape) == tuple(shape)
        rks = rk if hasattr(rk, "__len__") else [rk] * len(shape)
        assert [None if u is None else u.shape[1] for u in t.Us] == rks
    tb = tn.randn([3, 5, 6, 7], ranks_tucker=2, batch=True)
    assert [tuple(c.shape) for c in tb.cores] == [(3, 1, 2, 2), (3, 2, 2, 2), (3, 2, 2, 1)]


def test_ttmatrix_trace_sums_a_leading_rank():
    """matrix.py:160-175: the reference contracts from `ones(1)`, which einsum broadcasts over a leading boundary rank > 1,
    i.e. that rank is summed (round-2 advisor finding: row 0 only was taken)."""
    from tntorch_amd.matrix import TTMatrix

    torch.manual_seed(0)
    cores = [torch.randn(2, 3, 3, 4, dtype=torch.float64), torch.randn(4, 3, 3, 1, dtype=torch.float64)]
    m = TTMatrix.__new__(TTMatrix)
    m.cores, m.batch = cores, False
    want = torch.einsum("iaaj,jbbk->ik", cores[0], cores[1]).sum(dim=0)[0]
    assert abs(float(m.trace()) - float(want)) <= 1e-12


def test_verbose_prints_the_reference_stage_lines(capsys):
    """`verbose=True` prints the reference's per-stage timing lines (tensor.py:2032-2035; round.py:95-117, 163-185)."""
    t = tn.randn([6, 6, 6, 6], ranks_tt=5)
    t.round_tt(rmax=3, verbose=True)
    out = capsys.readouterr().out.splitlines()
    assert out[0].startswith("Orthogonalization time:")
    assert [ln.split(":")[0] for ln in out[1:]] == ["Time (SVD)", "Time (product)"] * 3
    t = tn.randn([6, 6, 6], ranks_tt=5)
    t.round_tt(eps=1e-3, algorithm="eig", verbose=True)
    out = capsys.readouterr().out.splitlines()
    assert [ln.split(":")[0] for ln in out] == ["Orthogonalization time"] + ["Time (gram)", "Time (symmetric EIG)", "Time (product)"] * 2
    tn.truncated_svd(torch.randn(9, 12), rmax=2, verbose=True)
    assert [ln.split(":")[0] for ln in capsys.readouterr().out.splitlines()] == ["Time (SVD)", "Time (product)"]
    t.round_tt(rmax=2)
    assert capsys.readouterr().out == ""


def test_idxs_are_built_on_first_use_and_travel_with_the_tensor():
    """tensor.py:433-435: `idxs` defaults to one arange per mode.  Here they are built on first access (N device launches per
    constructed tensor otherwise, on a latency-bound path); given ones are kept, clones share them, assignment works."""
    cores = oracle.tt_randn([3, 4, 5], 2, dtype=torch.float64)
    t = tn.Tensor([c.clone() for c in cores])
    assert t._idxs is None
    assert [i.tolist() for i in t.idxs] == [list(range(3)), list(range(4)), list(range(5))]
    assert t._idxs is not None and t.clone().idxs is t.idxs
    given = [torch.arange(3), torch.tensor([0, 1, 1, 0]), torch.arange(5)]
    u = tn.Tensor([c.clone() for c in cores], idxs=given)
    assert u.idxs is given and u.clone().idxs is given
    u.idxs = None
    assert [len(i) for i in u.idxs] == [3, 4, 5]

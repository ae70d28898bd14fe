"""tn.sparse_tt_svd on the CPU (the mirror the device path is compared with) and the argument envelope of its C entries.

The golden data (tests/golden/sparse_tt_svd_f64.npz, tools/gen_sparse_golden.py) are runs of the unmodified reference in fp64.
"""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import tntorch_amd as tn
from tntorch_amd import _hip, _hostops

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "sparse_tt_svd_f64.npz")
CASES = ("dense", "s200", "s200r", "n2")


def golden_case(name):
    z = np.load(GOLDEN)
    rmax = int(z[name + "_rmax"])
    return (torch.from_numpy(z[name + "_X"]), torch.from_numpy(z[name + "_y"]), float(z[name + "_eps"]), rmax or None,
            [int(r) for r in z[name + "_ranks"]], torch.from_numpy(z[name + "_recon"]))


def golden_bound(name):
    """Relative to ||y||: the larger of 100 x the worst distance of the CPU mirror from the reference's reconstruction over the
    golden cases (recorded in golden/sparse_tt_svd_meta.json when the mirror was written) and nrows x 2.2e-16, nrows the tallest unfolding."""
    with open(os.path.join(HERE, "golden", "sparse_tt_svd_meta.json")) as f:
        meta = json.load(f)
    X, y, eps, rmax, ranks, recon = golden_case(name)
    nrows = max(ranks[n] * recon.shape[n] for n in range(recon.dim() - 1))
    return max(100.0 * meta["mirror_worst_distance"], nrows * 2.2e-16)


def zero_filled(X, y, shape=None):
    shape = shape or [int(v) + 1 for v in X.max(dim=0)[0]]
    D = torch.zeros(shape, dtype=y.dtype)
    D[tuple(X.t())] = y
    return D


@pytest.mark.parametrize("name", CASES)
def test_golden_replay(name):
    X, y, eps, rmax, ranks, recon = golden_case(name)
    t = tn.sparse_tt_svd(X, y, eps, rmax=rmax)
    assert [int(r) for r in t.ranks_tt] == ranks
    assert t.cores[0].dtype == torch.float64
    dist = float(torch.norm(t.torch() - recon) / torch.norm(y))
    print(name, "distance from the reference's reconstruction / ||y|| =", dist, "bound", golden_bound(name))
    assert dist <= golden_bound(name)


@pytest.mark.parametrize("eps", [0.3, 0.05, 1e-6])
@pytest.mark.parametrize("name", ["dense", "s200"])
def test_eps_guarantee(name, eps):
    X, y = golden_case(name)[:2]
    t = tn.sparse_tt_svd(X, y, eps)
    D = zero_filled(X, y, [6, 5, 7, 4])
    err = float(torch.norm(t.torch() - D) / torch.norm(D))
    print(name, eps, "ranks", t.ranks_tt.tolist(), "relative error", err)
    assert err <= eps * (1 + 1e-6)


def test_rmax_caps_every_rank_and_shape_gives_zero_slices():
    X, y = golden_case("s200")[:2]
    for rmax in (1, 2, 5):
        t = tn.sparse_tt_svd(X, y, 1e-9, rmax=rmax)
        assert max(int(r) for r in t.ranks_tt) <= rmax
    shape = [8, 5, 9, 6]
    t = tn.sparse_tt_svd(X, y, 1e-9, shape=shape)
    assert list(t.shape) == shape
    full = t.torch()
    assert float(torch.norm(full - zero_filled(X, y, shape)) / torch.norm(y)) < 1e-12
    assert float(full[6:].abs().max()) == 0.0 and float(full[:, :, 7:].abs().max()) == 0.0 and float(full[..., 4:].abs().max()) == 0.0


def test_rank_is_capped_by_the_column_count():
    X, y = golden_case("s200")[:2]
    t = tn.sparse_tt_svd(X, y, 1e-9)
    assert int(t.ranks_tt[-2]) <= 4  # the last unfolding has at most 4 columns (the reference returns 64 here)
    cols = [len(torch.unique(X[:, n:], dim=0)) for n in range(1, 4)]
    assert all(int(t.ranks_tt[n + 1]) <= cols[n] for n in range(3))
    assert float(torch.norm(t.torch() - zero_filled(X, y, [6, 5, 7, 4])) / torch.norm(y)) < 1e-12


def test_value_errors():
    X = torch.tensor([[0, 1, 2], [1, 0, 1], [2, 2, 0]])
    y = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    bad = X.clone()
    bad[1, 2] = -1
    with pytest.raises(ValueError):
        tn.sparse_tt_svd(bad, y, 0.1)
    with pytest.raises(ValueError):
        tn.sparse_tt_svd(bad, y, 0.1, shape=[3, 3, 3])
    with pytest.raises(ValueError):
        tn.sparse_tt_svd(X, y, 0.1, shape=[3, 3, 2])  # index 2 in a mode of size 2
    with pytest.raises(ValueError):
        tn.sparse_tt_svd(torch.cat([X, X[:1]]), torch.cat([y, y[:1]]), 0.1)  # a repeated position
    with pytest.raises(ValueError):
        tn.sparse_tt_svd(X[:, :1], y, 0.1)  # N = 1
    with pytest.raises(ValueError):
        tn.sparse_tt_svd(X[:0], y[:0], 0.1)  # P = 0


def test_dtype_follows_y_and_numpy_inputs():
    X, y = golden_case("s200")[:2]
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float32)
    try:
        t64 = tn.sparse_tt_svd(X, y, 0.05)
        t32 = tn.sparse_tt_svd(X.numpy().astype(np.int32), y.numpy().astype(np.float32), 0.05)
    finally:
        torch.set_default_dtype(old)
    assert all(c.dtype == torch.float64 for c in t64.cores) and all(c.dtype == torch.float32 for c in t32.cores)
    D = zero_filled(X, y, [6, 5, 7, 4])
    assert float(torch.norm(t32.torch().double() - D) / torch.norm(D)) <= 0.05 * (1 + 1e-4)


def test_one_sample_and_two_modes():
    t = tn.sparse_tt_svd(torch.tensor([[2, 1]]), torch.tensor([3.0], dtype=torch.float64), 0.1, shape=[4, 3])
    full = t.torch()
    assert [int(r) for r in t.ranks_tt] == [1, 1, 1] and float(full[2, 1]) == pytest.approx(3.0, rel=1e-14)
    full[2, 1] = 0
    assert float(full.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------ C-ABI envelope
SPARSE_SIGNATURES = {
    "ttr_sparse_keys": ("c_int", ["c_long", "c_long", "c_void_p", "c_long", "c_long", "c_void_p", "c_void_p", "c_void_p", "c_void_p"]),
    "ttr_sparse_levels": ("c_int", ["c_long", "c_long", "c_void_p", "c_long", "c_long", "c_void_p", "c_void_p", "c_void_p", "c_void_p"]),
    "ttr_sparse_group_workspace_bytes": ("c_long", ["c_long", "c_long"]),
    "ttr_sparse_group": ("c_int", ["c_long", "c_long", "c_void_p", "c_void_p", "c_void_p", "c_void_p", "c_long", "c_void_p"]),
    "ttr_sparse_gram_parts": ("c_long", ["c_int", "c_long", "c_long", "c_long"]),
    "ttr_sparse_gram_workspace_bytes": ("c_long", ["c_int", "c_long", "c_long", "c_long"]),
    "ttr_sparse_gram": ("c_int", ["c_int"] + ["c_long"] * 4 + ["c_void_p"] * 6 + ["c_long", "c_void_p", "c_long", "c_void_p", "c_long", "c_void_p"]),
    "ttr_sparse_project": ("c_int", ["c_int"] + ["c_long"] * 5 + ["c_void_p"] * 3 + ["c_long", "c_void_p", "c_long", "c_long", "c_void_p", "c_long", "c_void_p"]),
}


def test_entries_are_declared_in_the_header():
    for name, (res, args) in SPARSE_SIGNATURES.items():
        got = _hip._SIGNATURES[name]
        assert (got[0].__name__, [a.__name__ for a in got[1]]) == (res, args), name
    assert _hip.ABI_VERSION >= 15


@pytest.fixture(scope="module")
def cabi():
    """The cross-compiled library, loaded without a device: every call below returns from its argument checks."""
    import __graft_entry__ as g

    g.build()
    L = ctypes.CDLL(g.LIB)
    for name in SPARSE_SIGNATURES:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = _hip._SIGNATURES[name]
    L.ttr_last_error.restype = ctypes.c_char_p
    return L


def test_sparse_entries_argument_envelope(cabi):
    OK, INVALID, UNSUPPORTED, WORKSPACE = _hip.OK, _hip.E_INVALID, _hip.E_UNSUPPORTED, _hip.E_WORKSPACE
    p = ctypes.c_void_p(64)  # never dereferenced: the calls below stop at their argument checks

    def gram(dt, r, I, nb, C, ptr=None, ldv=None, ldg=None, wsb=1 << 40):
        return cabi.ttr_sparse_gram(dt, r, I, nb, C, ptr, ptr, ptr, ptr, ptr, ptr, ldv or r, ptr, ldg or r * I, ptr, wsb, None)

    def project(dt, r, I, q, nb, C, ptr=None):
        return cabi.ttr_sparse_project(dt, r, I, q, nb, C, ptr, ptr, ptr, r, ptr, q, 1, ptr, q, None)

    assert cabi.ttr_sparse_keys(4, 3, None, 3, 1, None, None, None, None) == INVALID and b"NULL" in cabi.ttr_last_error()
    assert cabi.ttr_sparse_keys(4, 3, None, 3, 1, None, None, p, None) == INVALID and b"NULL" in cabi.ttr_last_error()
    assert cabi.ttr_sparse_keys(-1, 3, p, 3, 1, p, p, p, None) == INVALID and cabi.ttr_sparse_keys(4, 0, p, 3, 1, p, p, p, None) == INVALID
    assert cabi.ttr_sparse_levels(4, 3, None, 3, 1, None, None, None, None) == INVALID and b"NULL" in cabi.ttr_last_error()
    assert cabi.ttr_sparse_levels(0, 3, None, 3, 1, None, None, None, None) == OK
    assert cabi.ttr_sparse_levels(4, 0, p, 3, 1, p, p, p, None) == INVALID
    assert cabi.ttr_sparse_keys(1 << 31, 3, p, 3, 1, p, p, p, None) == UNSUPPORTED
    assert cabi.ttr_sparse_levels(1 << 31, 3, p, 3, 1, p, p, p, None) == UNSUPPORTED
    assert cabi.ttr_sparse_group_workspace_bytes(5000, 3) == 2 * 3 * 4 and cabi.ttr_sparse_group_workspace_bytes(0, 7) == 7 * 4
    assert cabi.ttr_sparse_group_workspace_bytes(10, 4097) == UNSUPPORTED and cabi.ttr_sparse_group_workspace_bytes(10, 0) == INVALID
    assert cabi.ttr_sparse_group(10, 3, None, None, None, None, 1 << 20, None) == INVALID and b"NULL" in cabi.ttr_last_error()
    assert cabi.ttr_sparse_group(10, 3, p, p, p, p, 11, None) == WORKSPACE
    assert cabi.ttr_sparse_group(10, 4097, p, p, p, p, 1 << 20, None) == UNSUPPORTED
    for dt, lim in ((_hip.F32, 4096), (_hip.F64, 2048)):
        assert cabi.ttr_eigh_max_n(dt) == lim
        assert gram(dt, 3, 5, 10, 4) == INVALID and b"NULL" in cabi.ttr_last_error()
        assert gram(dt, lim // 64 + 1, 64, 10, 4) == UNSUPPORTED and b"above" in cabi.ttr_last_error()
        assert gram(dt, 1, lim + 1, 10, 4) == UNSUPPORTED and gram(dt, lim, 1, 10, 4) == INVALID  # r I = limit: on to the pointers
        assert gram(dt, 0, 5, 10, 4) == INVALID and gram(dt, 3, 0, 10, 4) == INVALID and gram(dt, 3, 5, -1, 0) == INVALID
        assert gram(dt, 3, 5, 10, 11, p) == INVALID  # more columns than blocks
        assert gram(dt, 3, 5, 10, 4, p, ldv=2) == INVALID and gram(dt, 3, 5, 10, 4, p, ldg=14) == INVALID
        assert gram(dt, 3, 5, 10, 4, p, wsb=15 * 15 * (4 if dt == _hip.F32 else 8) - 1) == WORKSPACE
        assert gram(dt, 3, 5, 1 << 31, 4) == UNSUPPORTED
        assert cabi.ttr_sparse_gram_workspace_bytes(dt, 3, 5, 10) == 15 * 15 * (4 if dt == _hip.F32 else 8)
        assert cabi.ttr_sparse_gram_parts(dt, 3, 5, 10) == 1 and cabi.ttr_sparse_gram_parts(dt, 3, 1, 5000) == 3
        assert cabi.ttr_sparse_gram_parts(dt, lim + 1, 1, 10) == UNSUPPORTED
        assert project(dt, 3, 5, 2, 10, 4) == INVALID and b"NULL" in cabi.ttr_last_error()
        assert project(dt, 3, 5, 2, 10, 0) == OK
        assert project(dt, 3, 5, 16, 10, 4) == UNSUPPORTED  # q above r I
        assert project(dt, lim // 64 + 1, 64, 2, 10, 4) == UNSUPPORTED
        assert project(dt, 3, 5, 0, 10, 4) == INVALID and project(dt, 3, 5, 2, 3, 4) == INVALID
    assert gram(2, 3, 5, 10, 4) == INVALID and project(2, 3, 5, 2, 10, 4) == INVALID
    assert cabi.ttr_sparse_gram_parts(2, 3, 5, 10) == INVALID


# ------------------------------------------------------------------- the references and case lists of tests/sparse_cases.py
import sparse_cases as sc  # noqa: E402


def small_tables():
    yield sc.block_table([[0, 2], [], [1], [0, 1, 2], [2]], 2, torch.float64, 1)
    yield sc.block_table([[3]], 1, torch.float32, 2, I=5)
    yield sc.gram_table("passes_33", torch.float32)[0]
    yield sc.gram_table("passes_ragged_50", torch.float64)[0]
    yield sc.gram_table("geometry_Jt7", torch.float32)[0]
    yield sc.project_table("empty_columns", torch.float64)[0]


def test_block_table_against_loops():
    """colptr / blkcol / D element by element, D D^T as the column-by-column sum of the header's formula, and the two longest-sum
    lengths by counting."""
    for t in small_tables():
        r, I, C = t.r, t.I, t.C
        assert t.V.shape == (t.nb, r) and t.D.shape == (r * I, C) and t.D.dtype == torch.float64 and t.colptr.tolist()[-1] == t.nb
        D = [[0.0] * C for _ in range(r * I)]
        G = [[0.0] * (r * I) for _ in range(r * I)]
        holds = [set() for _ in range(I)]
        longest = 0
        for c in range(C):
            blocks = range(int(t.colptr[c]), int(t.colptr[c + 1]))
            longest = max(longest, len(blocks))
            for b in blocks:
                i = int(t.blk_i[b])
                assert int(t.blkcol[b]) == c
                holds[i].add(c)
                for a in range(r):
                    D[a * I + i][c] = float(t.V[b, a])
                for bp in blocks:  # G[(a,i),(b,j)] += V_ci[a] V_cj[b] over the columns that hold both
                    j = int(t.blk_i[bp])
                    for a in range(r):
                        for a2 in range(r):
                            G[a * I + i][a2 * I + j] += float(t.V[b, a]) * float(t.V[bp, a2])
        assert torch.equal(t.D, torch.tensor(D, dtype=torch.float64).reshape(r * I, C))
        ref = t.D @ t.D.t()
        G = torch.tensor(G, dtype=torch.float64)
        assert float((ref - G).abs().max()) <= 64 * 2.0**-53 * float(ref.abs().max())  # sums of at most 50 products, two orders
        assert t.gram_len == max(len(holds[i] & holds[j]) for i in range(I) for j in range(I))
        assert t.project_len == r * longest


def test_group_reference_against_a_loop():
    for nb, I, kind in [(0, 3, "random"), (1, 1, "random"), (300, 7, "random"), (300, 7, "one_index"), (500, 20, "out_of_range")]:
        b = sc.group_input(nb, I, kind).tolist()
        ilist, iptr = sc.group_reference(b, I)
        order, ptr = [], [0]
        for i in range(I):
            order += [k for k, v in enumerate(b) if v == i]
            ptr.append(len(order))
        assert ilist.tolist() == order and iptr.tolist() == ptr
        if kind == "out_of_range":
            assert len(order) < nb and set(b) - set(range(I)) == {I, I + 1}


def test_keys_and_levels_references_against_loops():
    for shape in (sc.KEYS_SHAPES[1], sc.KEYS_SHAPES[4], sc.KEYS_BIG_SHAPE):
        X = sc.keys_input(shape, 3, P=40, corners=len(shape) == 3)
        keys = sc.keys_reference(X, shape)
        weights = [math.prod(shape[:n]) for n in range(len(shape))]  # x_1 minor
        assert keys == [sum(int(x) * w for x, w in zip(row, weights)) for row in X.tolist()]
        assert all(0 <= k < math.prod(shape) for k in keys)
        # the key order is the order of the reversed tuples
        assert sorted(range(40), key=lambda p: keys[p]) == sorted(range(40), key=lambda p: (X[p].tolist()[::-1], p))
    for N in (1, 4):
        for rotation in range(N):
            levs = sc.level_sequence(N, rotation)
            Xs = sc.sorted_set(levs, N, 5)
            rows = Xs.tolist()
            assert all(a[::-1] < b[::-1] for a, b in zip(rows, rows[1:]))  # strictly ascending, x_N major
            brute = [N] + [max([n + 1 for n in range(N) if a[n] != b[n]], default=0) for a, b in zip(rows, rows[1:])]
            assert sc.levels_reference(Xs.numpy()).tolist() == brute == levs
            X, perm = sc.shuffled(Xs, 6)
            assert torch.equal(X[perm.long()], Xs)
    Xs[256] = Xs[255]
    assert sc.levels_reference(Xs.numpy())[256] == 0
    edges = {p: {sc.level_sequence(4, s)[p] for s in range(4)} for p in sc.LEVEL_EDGES}
    assert all(v == {1, 2, 3, 4} for v in edges.values())  # every edge sees every level


@pytest.mark.parametrize("name", list(sc.CANONICAL_CASES))
def test_host_canonical_against_sorted_tuples(name):
    shape, P = sc.CANONICAL_CASES[name]
    X = sc.distinct_positions(shape, P, 100 + len(name))
    rows = X.tolist()
    assert len(set(map(tuple, rows))) == P and all(0 <= x < s for row in rows for x, s in zip(row, shape))
    perm, lev = _hostops.sparse_canonical(X, shape)
    assert perm.dtype == torch.int32 and lev.dtype == torch.int32
    assert perm.tolist() == sorted(range(P), key=lambda p: rows[p][::-1])
    assert lev.tolist() == sc.levels_reference(X[perm.long()].numpy()).tolist()
    if math.prod(shape) < 2**63:  # the order of the linear keys, where they fit
        keys = sc.keys_reference(X, shape)
        assert perm.tolist() == sorted(range(P), key=lambda p: keys[p])


def test_case_lists_build_valid_tables():
    for name, (r, I, cols, parts) in sc.GRAM_CASES.items():
        assert sc.valid_columns(cols, I) and all(len(c) > 0 for c in cols), name
        nb = sum(len(c) for c in cols)
        assert parts == sc.gram_parts(I, nb) and (parts > 1) == (name in sc.PARTS_CASES), name
        lens = [sum(i in c for c in cols) for i in range(I)]
        if name.startswith("passes"):
            assert min(lens) > sc.KCH and all(len(c) >= 2 for c in cols), (name, lens)  # several passes, partners everywhere
    lens = {n: [sum(i in c for c in sc.GRAM_CASES[n][2]) for i in range(sc.GRAM_CASES[n][1])] for n in sc.GRAM_CASES}
    assert lens["passes_33"] == [33] * 3 and lens["passes_64"] == [64] * 3 and lens["passes_65"] == [65] * 3
    assert lens["passes_ragged_50"] == [33, 33, 34] and lens["passes_ragged_98"] == [65, 65, 66]
    assert lens["parts_short_absent"] == [5124, 5122, 4, 1, 0] and sum(lens["parts_short_absent"]) > 2048 * 5
    assert sum(lens["parts_partners"]) == 4098 and sum(lens["parts_cap"]) > 16 * 2048 * 2
    for name in ("geometry_I200", "geometry_I130"):
        r, I, cols, _ = sc.GRAM_CASES[name]
        assert len(cols) == 42 and sum(len(c) == I for c in cols) == 2 and -(-I // 64) >= 3  # column scans of three strides
    for name, (cols, q) in sc.PROJECT_CASES.items():
        assert sc.valid_columns(cols, sc.PROJECT_I) and 1 <= q <= sc.PROJECT_R * sc.PROJECT_I, name
        assert all(len(c) > 0 for c in cols) or name == "empty_columns"
    assert sorted(len(c) for c, q in sc.PROJECT_CASES.values() if q == 7) == [1, 23, 35, 36, 37, 40] and sc.project_cpw(7) == 36
    assert sorted(len(c) for c, q in sc.PROJECT_CASES.values() if q == 1) == [23, 255, 256, 257] and sc.project_cpw(1) == 256
    assert [sc.canonical_branch(s) for s, _ in sc.CANONICAL_CASES.values()] == ["int32", "int32", "int64", "no_keys"]
    for name in sc.END_TO_END_CASES:
        shape = sc.END_TO_END_CASES[name][0]
        X, y, Z = sc.end_to_end_samples(name)
        assert sc.canonical_branch(shape) == name and X.shape == (300, len(shape)) == Z.shape
        rows = set(map(tuple, X.tolist()))
        assert len(rows) == 300 and not rows & set(map(tuple, Z.tolist()))
        assert all(0 <= int(A[:, n].min()) and int(A[:, n].max()) < shape[n] for A in (X, Z) for n in range(len(shape)))
        t = tn.sparse_tt_svd(X, y, 1e-6, shape=shape)  # the CPU mirror: a rank-2 tensor, zero off the grid
        assert max(int(r) for r in t.ranks_tt) == 2
        assert float(torch.norm(sc.evaluate(t.cores, X) - y) / torch.norm(y)) <= 1e-6 and float(torch.norm(sc.evaluate(t.cores, Z)) / torch.norm(y)) <= 1e-6


def test_declared_part_counts_match_the_library(cabi):
    for name, (r, I, cols, parts) in sc.GRAM_CASES.items():
        nb = sum(len(c) for c in cols)
        for dt in (_hip.F32, _hip.F64):
            assert cabi.ttr_sparse_gram_parts(dt, r, I, nb) == parts, name
    assert cabi.ttr_sparse_group_workspace_bytes(*sc.GROUP_BIG) == 966 * 3 * 4
    assert cabi.ttr_sparse_group_workspace_bytes(4194304, 3) == 1024 * 3 * 4  # chunks of 4096 blocks up to here

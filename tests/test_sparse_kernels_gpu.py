"""The kernels of csrc/ttr_sparse.hip at their pass, part, tile and key edges, each against a plain reference on the CPU
(tests/sparse_cases.py, whose references tests/test_sparse_host.py checks against brute-force loops):
- ttr_sparse_gram against D D^T in fp64: i lists of 33, 64, 65 blocks whose every block has partners at other indices (several
  passes of 32 blocks with the accumulators carried over), ragged lists, lists split into 2 and 16 parts with off-diagonal blocks, a
  list shorter than the part count and an absent index, three rank tiles, four j ranges, j ranges of 7 and 4, ldv > r, ldg > r I;
- ttr_sparse_project against D^T U[:, :q]: q on both sides of 256, C on both sides of a multiple of the columns per workgroup,
  empty columns, U in three layouts, V as a column slice, ldw > q;
- ttr_sparse_group against a stable sort: sizes around the 256-block tile and the 4096-block chunk, 1 to 4096 bins, one index
  only, a chunk above 4096 blocks, entries outside [0, I);
- ttr_sparse_keys / ttr_sparse_levels: several workgroups, strided X, N = 1, keys up to 2^62 - 1, the validation kernel's
  grid-stride tail, levels and a repeated position at a workgroup boundary, a perm entry out of range;
- _hipops.sparse_canonical against _hostops.sparse_canonical in its three branches (int32 keys, int64 keys, no keys), and
  tn.sparse_tt_svd end to end in each.
Bounds are those of tests/test_sparse_gpu.py: L u max |G_ref| for the Gram matrix and L u (|D|^T |U|) elementwise for the
projection, u the unit roundoff, L the exact longest sum of the table (plus the part count where a list is split).
No case hands a kernel an index that it could turn into an access out of bounds: the group cases use I and I + 1 with I = 1000 (inside
the 4096-entry LDS arrays whatever the kernel does), the perm = P case is refused by the guard at the top of sparse_levels_kernel,
and gram / project only see valid tables."""
import numpy as np
import pytest
import torch

import sparse_cases as sc
import tntorch_amd as tn
from tntorch_amd import _hip, _hipops, _hostops

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.float64]
EPS = {torch.float32: 2.0**-24, torch.float64: 2.0**-53}  # unit roundoff
SENTINEL = -7.5


def dev32(a):
    return a.to(DEV, torch.int32)


def check_group(blk_i, I):
    """ttr_sparse_group on int32 ``blk_i`` (CPU) against the stable sort; returns the device (ilist, iptr)."""
    ilist, iptr = _hip.sparse_group(blk_i.to(DEV), I)
    order, ptr = sc.group_reference(blk_i.numpy(), I)
    assert ilist.dtype == torch.int32 and iptr.dtype == torch.int32 and ilist.shape[0] == blk_i.shape[0] and iptr.shape[0] == I + 1
    assert np.array_equal(iptr.cpu().numpy(), ptr), (blk_i.shape[0], I)
    assert np.array_equal(ilist.cpu().numpy()[: int(ptr[-1])], order), (blk_i.shape[0], I)
    return ilist, iptr


def device_gram(t, V=None):
    ilist, iptr = check_group(t.blk_i.to(torch.int32), t.I)
    return _hip.sparse_gram(t.V.to(DEV) if V is None else V, t.I, dev32(t.colptr), dev32(t.blk_i), dev32(t.blkcol), ilist, iptr)


def device_project(t, U, q, V=None):
    return _hip.sparse_project(t.V.to(DEV) if V is None else V, t.I, dev32(t.colptr), dev32(t.blk_i), U, q)


def wide_slice(V, left, right):
    """V as a column slice of a wider device tensor (row stride r + left + right)."""
    nb, r = V.shape
    wide = torch.randn(nb, r + left + right, generator=torch.Generator().manual_seed(3), dtype=torch.float64).to(V.dtype)
    wide[:, left : left + r] = V
    Vd = wide.to(DEV)[:, left : left + r]
    assert Vd.stride(0) == r + left + right and Vd.stride(1) == 1
    return Vd


# --------------------------------------------------------------------------------------------------------------------- gram
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(sc.GRAM_CASES))
def test_gram_against_dense(name, dtype):
    t, ref = sc.gram_table(name, dtype)
    parts = sc.GRAM_CASES[name][3]
    assert _hip.sparse_gram_parts(dtype, t.r, t.I, t.nb) == parts == sc.gram_parts(t.I, t.nb)
    G = device_gram(t)
    L = t.gram_len + (parts if parts > 1 else 0)
    err, bound = float((G.cpu().double() - ref).abs().max()), L * EPS[dtype] * float(ref.abs().max())
    print(name, dtype, "nb", t.nb, "parts", parts, "L", L, "err", err, "bound", bound)
    assert err <= bound, (name, err, bound)
    assert torch.equal(G, G.t()), name
    assert torch.equal(G, device_gram(t)), name  # run to run
    absent = torch.bincount(t.blk_i, minlength=t.I) == 0
    assert bool(absent.any()) == (name == "parts_short_absent")
    if bool(absent.any()):
        rows = (torch.arange(t.r)[:, None] * t.I + torch.nonzero(absent)[:, 0][None, :]).reshape(-1).to(DEV)
        assert float(G[rows].abs().max()) == 0.0 and float(G[:, rows].abs().max()) == 0.0, name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["passes_65", "parts_partners", "geometry_Jt7", "geometry_r65"])
def test_gram_leading_dimensions(name, dtype):
    """ldv > r through the binding (V a column slice), ldg = r I + 3 through the C entry: the same bits, the pad untouched."""
    t, ref = sc.gram_table(name, dtype)
    G = device_gram(t)
    Vd = wide_slice(t.V, 0, 3)
    assert torch.equal(device_gram(t, Vd), G), name
    n, ldg = t.r * t.I, t.r * t.I + 3
    ilist, iptr = _hip.sparse_group(dev32(t.blk_i), t.I)
    colptr, blk_i, blkcol = dev32(t.colptr), dev32(t.blk_i), dev32(t.blkcol)
    dt = _hip.dtype_code(dtype)
    wsb = int(_hip.lib().ttr_sparse_gram_workspace_bytes(dt, t.r, t.I, t.nb))
    assert wsb == sc.GRAM_CASES[name][3] * n * n * (4 if dtype == torch.float32 else 8)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    out = torch.full((n, ldg), SENTINEL, dtype=dtype, device=DEV)
    _hip._call("ttr_sparse_gram", dt, t.r, t.I, t.nb, t.C, colptr.data_ptr(), blk_i.data_ptr(), blkcol.data_ptr(), ilist.data_ptr(),
               iptr.data_ptr(), Vd.data_ptr(), int(Vd.stride(0)), out.data_ptr(), ldg, ws.data_ptr(), wsb)
    assert torch.equal(out[:, :n], G), name
    assert bool((out[:, n:] == SENTINEL).all()), name


# ------------------------------------------------------------------------------------------------------------------ project
def column_major(U):
    return U.t().contiguous().to(DEV).t()


def check_project(t, q, W, ref, scale, dtype, what):
    assert W.shape == (t.C, q)
    excess = float(((W.cpu().double() - ref).abs() - t.project_len * EPS[dtype] * scale).max())
    print(what, dtype, "C", t.C, "q", q, "L", t.project_len, "worst error above its bound", excess)
    assert bool(((W.cpu().double() - ref).abs() <= t.project_len * EPS[dtype] * scale + 1e-300).all()), what


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(sc.PROJECT_CASES))
def test_project_against_dense(name, dtype):
    t, q, ref, scale = sc.project_table(name, dtype)
    U = column_major(sc.project_matrix(dtype))
    W = device_project(t, U, q)
    check_project(t, q, W, ref, scale, dtype, name)
    assert torch.equal(W, device_project(t, U, q)), name  # run to run
    empty = torch.nonzero(t.colptr[1:] == t.colptr[:-1])[:, 0]
    assert (empty.numel() > 0) == (name == "empty_columns")
    if empty.numel():
        assert empty.tolist() == [0, 17, 35, 36, 39] and float(W[empty.to(DEV)].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["q1", "q7", "q257", "empty_columns"])
def test_project_layouts(name, dtype):
    """U column-major (as the eigensolver leaves it), row-major with more than q columns, row-major with exactly q columns; V a
    column slice; ldw = q + 5 through the C entry.  One fma chain per element whatever the strides: the same bits."""
    t, q, ref, scale = sc.project_table(name, dtype)
    Uh = sc.project_matrix(dtype)
    n = Uh.shape[0]
    W = device_project(t, column_major(Uh), q)
    check_project(t, q, W, ref, scale, dtype, name)
    Urow, Uexact = Uh.contiguous().to(DEV), Uh[:, :q].contiguous().to(DEV)
    assert Urow.stride() == (n, 1) and Uexact.shape == (n, q) and Uexact.is_contiguous() and n > q
    assert torch.equal(device_project(t, Urow, q), W), name
    assert torch.equal(device_project(t, Uexact, q), W), name
    Vd = wide_slice(t.V, 1, 2)
    assert torch.equal(device_project(t, Urow, q, Vd), W), name
    ldw = q + 5
    colptr, blk_i = dev32(t.colptr), dev32(t.blk_i)
    out = torch.full((t.C, ldw), SENTINEL, dtype=dtype, device=DEV)
    _hip._call("ttr_sparse_project", _hip.dtype_code(dtype), t.r, t.I, q, t.nb, t.C, colptr.data_ptr(), blk_i.data_ptr(), Vd.data_ptr(),
               int(Vd.stride(0)), Urow.data_ptr(), n, 1, out.data_ptr(), ldw)
    assert torch.equal(out[:, :q], W), name
    assert bool((out[:, q:] == SENTINEL).all()), name


# -------------------------------------------------------------------------------------------------------------------- group
@pytest.mark.parametrize("I", sc.GROUP_I)
@pytest.mark.parametrize("nb", sc.GROUP_NB)
def test_group_sizes(nb, I):
    check_group(sc.group_input(nb, I), I)


def test_group_one_index_fills_every_tile():
    """600 blocks at one index: two full tiles of 256 whose every thread ranks itself among 255 others, and a tail."""
    ilist, iptr = check_group(sc.group_input(600, 7, "one_index"), 7)
    assert iptr.tolist() == [0] * 4 + [600] * 4 and ilist.tolist() == list(range(600))


def test_group_chunk_above_4096_blocks():
    nb, I = sc.GROUP_BIG
    assert nb > 1024 * 4096 and int(_hip.lib().ttr_sparse_group_workspace_bytes(nb, I)) == 966 * I * 4  # chunks of 4352 blocks
    check_group(sc.group_input(nb, I), I)


def test_group_leaves_out_of_range_entries_out():
    b = sc.group_input(10000, 1000, "out_of_range")
    outside = int((b >= 1000).sum())
    assert outside > 1000 and int(b.max()) == 1001 and bool((b == 1000).any())
    ilist, iptr = check_group(b, 1000)
    assert int(iptr[1000]) == 10000 - outside


# ---------------------------------------------------------------------------------------------------------- keys and levels
def layouts(X, pad=-99):
    """X on the device: contiguous, as the transposed view of an [N, P] matrix, and as a column slice of a wider matrix whose other
    columns hold invalid indices."""
    P, N = X.shape
    wide = torch.full((P, N + 3), pad, dtype=torch.int64)
    wide[:, 2 : 2 + N] = X
    views = [("contiguous", X.contiguous().to(DEV)), ("transposed", X.t().contiguous().to(DEV).t()),
             ("column slice", wide.to(DEV)[:, 2 : 2 + N])]
    assert (N == 1 or views[1][1].stride() == (1, P)) and views[2][1].stride() == (N + 3, 1)  # (one column has no transposed view)
    return views


def device_keys(Xd, shape):
    flag = torch.full((1,), 7, dtype=torch.int32, device=DEV)  # the entry clears it
    key = _hip.sparse_keys(Xd, torch.tensor(shape, dtype=torch.int64, device=DEV), flag)
    return key, int(flag)


def device_levels(Xd, perm):
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    lev = _hip.sparse_levels(Xd, perm.to(DEV), flag)
    return lev, int(flag)


@pytest.mark.parametrize("N", [1, 4])
def test_keys_and_levels_over_workgroups_and_strides(N):
    shape = sc.KEYS_SHAPES[N]
    X = sc.keys_input(shape, 40 + N)
    expect = sc.keys_reference(X, shape)
    for what, Xd in layouts(X):
        key, flag = device_keys(Xd, shape)
        assert flag == 0 and key.tolist() == expect, (N, what)
    levs = sc.level_sequence(N, 0)
    Xs = sc.sorted_set(levs, N, 50 + N)
    X, perm = sc.shuffled(Xs, 60 + N)
    expect = sc.levels_reference(Xs.numpy())
    assert expect.tolist() == levs
    for what, Xd in layouts(X):
        lev, flag = device_levels(Xd, perm)
        assert flag == 0 and np.array_equal(lev.cpu().numpy(), expect), (N, what)


def test_keys_up_to_2_62():
    shape = sc.KEYS_BIG_SHAPE
    X = sc.keys_input(shape, 44, corners=True)
    expect = sc.keys_reference(X, shape)
    assert max(expect) == 2**62 - 1 and min(expect) == 0 and 2**62 - 2**41 in expect  # (0, 0, I_3 - 1)
    for what, Xd in layouts(X):
        key, flag = device_keys(Xd, shape)
        assert flag == 0 and key.tolist() == expect, what


_VALID = {}


def validation_input():
    if not _VALID:
        X = sc.keys_input(sc.VALIDATE_SHAPE, 45, P=sc.VALIDATE_P)
        s = sc.VALIDATE_SHAPE
        _VALID["X"], _VALID["key"] = X.to(DEV), ((X[:, 3] * s[2] + X[:, 2]) * s[1] + X[:, 1]) * s[0] + X[:, 0]
    return _VALID["X"], _VALID["key"]


def test_validation_passes_a_clean_input_past_its_grid():
    X, expect = validation_input()
    assert X.numel() > sc.VALIDATE_GRID_ELEMS
    key, flag = device_keys(X, sc.VALIDATE_SHAPE)
    assert flag == 0 and torch.equal(key.cpu(), expect)


@pytest.mark.parametrize("value", ["negative", "size"])
@pytest.mark.parametrize("elem", sc.VALIDATE_ELEMS)
def test_validation_grid_stride_tail(elem, value):
    """One bad index, in the last element and in the first element that only the grid-stride loop's second trip reaches."""
    X, _ = validation_input()
    p, n = divmod(elem, 4)
    assert p < sc.VALIDATE_P and elem >= sc.VALIDATE_GRID_ELEMS
    bad = X.clone()
    bad[p, n] = -1 if value == "negative" else sc.VALIDATE_SHAPE[n]
    flag = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    key = torch.full((sc.VALIDATE_P,), -5, dtype=torch.int64, device=DEV)
    shape = torch.tensor(sc.VALIDATE_SHAPE, dtype=torch.int64, device=DEV)
    _hip._call("ttr_sparse_keys", sc.VALIDATE_P, 4, bad.data_ptr(), 4, 1, shape.data_ptr(), key.data_ptr(), flag.data_ptr())
    assert int(flag) == 1 and bool((key == -5).all())


@pytest.mark.parametrize("rotation", range(4))
def test_levels_at_workgroup_boundaries(rotation):
    levs = sc.level_sequence(4, rotation)
    assert [levs[p] for p in sc.LEVEL_EDGES] == [1 + (k + rotation) % 4 for k in range(4)]
    Xs = sc.sorted_set(levs, 4, 70 + rotation)
    X, perm = sc.shuffled(Xs, 80 + rotation)
    lev, flag = device_levels(X.to(DEV), perm)
    assert flag == 0 and lev.tolist() == levs == sc.levels_reference(Xs.numpy()).tolist()


def test_one_repeated_position_at_a_workgroup_boundary():
    Xs = sc.sorted_set(sc.level_sequence(4, 1), 4, 90)
    Xs[256] = Xs[255]
    expect = sc.levels_reference(Xs.numpy())
    assert expect[256] == 0 and int((expect == 0).sum()) == 1
    X, perm = sc.shuffled(Xs, 91)
    lev, flag = device_levels(X.to(DEV), perm)
    assert flag == 2 and int(lev[256]) == 0 and np.array_equal(lev.cpu().numpy(), expect)


def test_perm_entry_out_of_range_sets_bit_0():
    """perm[300] = P is refused by the guard at the top of sparse_levels_kernel (r0 >= P): no row of X is read through it."""
    Xs = sc.sorted_set(sc.level_sequence(4, 2), 4, 92)
    X, perm = sc.shuffled(Xs, 93)
    perm = perm.clone()
    perm[300] = X.shape[0]
    lev, flag = device_levels(X.to(DEV), perm)
    assert flag & 1


# --------------------------------------------------------------------------------------------------------- sparse_canonical
def test_case_shapes_reach_every_branch():
    assert [sc.canonical_branch(s) for s, _ in sc.CANONICAL_CASES.values()] == ["int32", "int32", "int64", "no_keys"]
    assert [sc.canonical_branch(s) for s, _ in sc.END_TO_END_CASES.values()] == ["int32", "int64", "no_keys"]


def spy_on_keys(monkeypatch):
    """Record (want_keys, sort key dtype) of the sparse_canonical calls that follow."""
    seen = []
    keys, sort = _hip.sparse_keys, torch.sort

    def sparse_keys(X, shape_dev, flag, want_keys=True):
        seen.append(["keys" if want_keys else "no_keys"])
        return keys(X, shape_dev, flag, want_keys=want_keys)

    def spy_sort(a, *args, **kw):
        if seen and len(seen[-1]) == 1 and seen[-1][0] == "keys":
            seen[-1].append(a.dtype)
        return sort(a, *args, **kw)

    monkeypatch.setattr(_hip, "sparse_keys", sparse_keys)
    monkeypatch.setattr(torch, "sort", spy_sort)
    return seen


BRANCH_TRACE = {"int32": ["keys", torch.int32], "int64": ["keys", torch.int64], "no_keys": ["no_keys"]}


@pytest.mark.parametrize("name", list(sc.CANONICAL_CASES))
def test_canonical_device_against_host(name, monkeypatch):
    shape, P = sc.CANONICAL_CASES[name]
    X = sc.distinct_positions(shape, P, 100 + len(name))
    assert X.shape == (P, len(shape)) and len(set(map(tuple, X.tolist()))) == P
    assert all(int(X[:, n].max()) == shape[n] - 1 and int(X[:, n].min()) == 0 for n in range(len(shape)))
    perm_h, lev_h = _hostops.sparse_canonical(X, shape)
    seen = spy_on_keys(monkeypatch)
    perm_d, lev_d = _hipops.sparse_canonical(X.to(DEV), shape)
    monkeypatch.undo()
    print(name, "shape", shape, "branch", seen)
    assert seen == [BRANCH_TRACE[sc.canonical_branch(shape)]]
    assert perm_d.dtype == torch.int32 and lev_d.dtype == torch.int32
    assert torch.equal(perm_d.cpu(), perm_h) and torch.equal(lev_d.cpu(), lev_h)


@pytest.mark.parametrize("eps", [0.3, 0.05])
@pytest.mark.parametrize("name", list(sc.END_TO_END_CASES))
def test_end_to_end_in_every_branch(name, eps, monkeypatch):
    """The guarantee of test_sparse_gpu.test_eps_guarantee_fp32, with the error taken over the samples and 300 held-out zero
    positions (a part of the full error, which the dense tensor would be needed for)."""
    shape = sc.END_TO_END_CASES[name][0]
    X, y, Z = sc.end_to_end_samples(name)
    y = y.float()
    seen = spy_on_keys(monkeypatch)
    t = tn.sparse_tt_svd(X.to(DEV), y.to(DEV), eps, shape=shape)
    monkeypatch.undo()
    assert seen == [BRANCH_TRACE[name]]
    assert all(c.is_cuda and c.dtype == torch.float32 for c in t.cores) and list(t.shape) == shape
    assert max(int(r) for r in t.ranks_tt) <= 2
    at_samples, at_zeros = sc.evaluate(t.cores, X) - y.double(), sc.evaluate(t.cores, Z)
    err = float(torch.sqrt((at_samples**2).sum() + (at_zeros**2).sum()) / torch.norm(y.double()))
    print(name, eps, "ranks", t.ranks_tt.tolist(), "relative error over samples and held-out zeros", err)
    assert err <= eps * (1 + 1e-6)

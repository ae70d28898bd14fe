"""Inputs, named cases and plain references for the kernels of ``tntorch_amd/csrc/ttr_sparse.hip`` (keys, levels, group, gram,
project), shared by tests/test_sparse_host.py (which checks every reference here against a brute-force loop, on the CPU) and
tests/test_sparse_kernels_gpu.py.  Nothing here touches a device.

The constants mirror the kernels' documented geometry: a Gram workgroup walks an i list 32 blocks per pass (kCh), a list is split
into min(16, ceil(nb / (2048 I))) parts, a project workgroup owns cpw = 256 // min(q, 256) columns, the group kernels hold at most
4096 bins and rank 256 blocks per tile, and the validation kernel's grid stops at 4096 workgroups of 256 threads."""
import collections
import itertools
import math

import numpy as np
import torch

KCH, PART_BLOCKS, MAX_PARTS, THREADS, GROUP_MAX_I = 32, 2048, 16, 256, 4096
VALIDATE_GRID_ELEMS = 4096 * THREADS  # the validation kernel's grid-stride tail starts at this flat element

Table = collections.namedtuple("Table", "colptr blk_i blkcol V D r I C nb gram_len project_len")


def block_table(cols, r, dtype, seed, I=None):
    """The block table of the explicit per-column index lists ``cols`` (each ascending, every index at most once; an empty list is
    a column without blocks) with random values: int64 colptr [C + 1], blk_i [nb], blkcol [nb], V [nb, r] in ``dtype`` and the dense
    D [r I, C] in fp64 built from the rounded V (D[a I + i, c] = V[b, a] for block b of column c at mode index i).  ``gram_len`` is
    the exact longest sum of D D^T, the largest number of columns that hold both i and j over all pairs (i, j); ``project_len`` the
    longest sum of D^T U, r times the longest column.  ``I`` defaults to the largest index + 1."""
    C = len(cols)
    counts = torch.tensor([len(c) for c in cols], dtype=torch.int64)
    blk_i = torch.tensor([i for c in cols for i in c], dtype=torch.int64)
    nb = int(blk_i.numel())
    I = int(I) if I is not None else int(blk_i.max()) + 1
    colptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(counts, 0)])
    blkcol = torch.repeat_interleave(torch.arange(C), counts)
    g = torch.Generator().manual_seed(seed)
    V = torch.randn(nb, r, generator=g, dtype=torch.float64).to(dtype)
    D = torch.zeros(r * I, C, dtype=torch.float64)
    D[torch.arange(r)[None, :] * I + blk_i[:, None], blkcol[:, None].expand(-1, r)] = V.double()
    M = torch.zeros(I, C, dtype=torch.float64)  # M[i, c] = 1: column c holds index i
    M[blk_i, blkcol] = 1.0
    gram_len = int((M @ M.t()).max()) if nb else 0
    return Table(colptr, blk_i, blkcol, V, D, r, I, C, nb, gram_len, r * int(counts.max()) if C else 0)


def valid_columns(cols, I):
    """Indices inside [0, I), strictly ascending within every column (so at most once each)."""
    return all(all(0 <= i < I for i in c) and all(a < b for a, b in zip(c, c[1:])) for c in cols)


def gram_parts(I, nb):
    """The documented part count of ttr_sparse_gram (below the 256 MiB budget of the partial matrices, which no case here nears)."""
    return min(MAX_PARTS, max(1, -(-nb // (PART_BLOCKS * I))))


def project_cpw(q):
    return THREADS // min(q, THREADS)


def _random_columns(I, C, mmax, seed):
    g = torch.Generator().manual_seed(seed)
    cols = []
    for _ in range(C):
        m = int(torch.randint(1, min(I, mmax) + 1, (1,), generator=g))
        cols.append(sorted(torch.randperm(I, generator=g)[:m].tolist()))
    return cols


def _full(I, C):
    return [list(range(I)) for _ in range(C)]


def _ragged(I, C):
    """Column c holds every index but c mod I."""
    return [[i for i in range(I) if i != c % I] for c in range(C)]


def _with_full(I, C, mmax, seed, at):
    cols = _random_columns(I, C, mmax, seed)
    for c in at:
        cols[c] = list(range(I))
    return cols


# name -> (r, I, columns, part count).  Passes: lists of 32 + 1, 64 and 64 + 1 blocks whose every block has I partners; the ragged
# tables need 50 and 98 columns for lists of 33 / 33 / 34 and 65 / 65 / 66 (a column drops one index of three).  Parts: two parts
# with partners; a split with a list of one block (its second part is empty) and an absent index; the cap of 16 parts.  Geometry:
# three rank tiles (r = 65), four j ranges scanned in three strides of 64 blocks (I = 200, 130 with two full columns), j ranges of
# 7 and 4 (r = 17, 22 at I = 9).
GRAM_CASES = collections.OrderedDict()
for _C in (33, 64, 65):
    GRAM_CASES["passes_{}".format(_C)] = (2, 3, _full(3, _C), 1)
for _C in (50, 98):
    GRAM_CASES["passes_ragged_{}".format(_C)] = (2, 3, _ragged(3, _C), 1)
GRAM_CASES["parts_partners"] = (3, 2, _full(2, 2049), 2)
GRAM_CASES["parts_short_absent"] = (2, 5, [[0, 1]] * (PART_BLOCKS * 5 // 2 + 1) + [[0, 2]] * 3 + [[1, 2, 3]], 2)
GRAM_CASES["parts_cap"] = (2, 2, _full(2, MAX_PARTS * PART_BLOCKS + 1), 16)
GRAM_CASES["geometry_r65"] = (65, 3, _with_full(3, 9, 3, 65, (4,)), 1)
GRAM_CASES["geometry_I200"] = (1, 200, _with_full(200, 42, 12, 200, (5, 30)), 1)
GRAM_CASES["geometry_I130"] = (2, 130, _with_full(130, 42, 12, 130, (0, 41)), 1)
GRAM_CASES["geometry_Jt7"] = (17, 9, _with_full(9, 13, 5, 17, (6,)), 1)
GRAM_CASES["geometry_Jt4"] = (22, 9, _with_full(9, 13, 5, 22, (6,)), 1)
PARTS_CASES = ("parts_partners", "parts_short_absent", "parts_cap")

# name -> (columns, q) at r = 5, I = 64: q on both sides of the 256 threads of a workgroup; C on both sides of a multiple of cpw
# (36 columns per workgroup at q = 7, 256 at q = 1); one column; empty columns first, in the middle, last and at a workgroup edge
PROJECT_R, PROJECT_I = 5, 64
PROJECT_CASES = collections.OrderedDict()
for _q in (1, 7, 255, 256, 257, 300):
    PROJECT_CASES["q{}".format(_q)] = (_random_columns(PROJECT_I, 23, 6, 500 + _q), _q)
for _q in (7, 1):
    for _d in (-1, 0, 1):
        _C = project_cpw(_q) + _d
        PROJECT_CASES["q{}_C{}".format(_q, _C)] = (_random_columns(PROJECT_I, _C, 6, 600 + _C), _q)
PROJECT_CASES["one_column"] = (_random_columns(PROJECT_I, 1, 6, 700), 7)
_cols = _random_columns(PROJECT_I, 40, 6, 701)
for _c in (0, 17, 35, 36, 39):
    _cols[_c] = []
PROJECT_CASES["empty_columns"] = (_cols, 7)

_TABLES = {}


def gram_table(name, dtype):
    """The table of a Gram case and its fp64 D D^T, built once: (Table, ref)."""
    key = ("gram", name, dtype)
    if key not in _TABLES:
        r, I, cols, _ = GRAM_CASES[name]
        t = block_table(cols, r, dtype, 1000 + list(GRAM_CASES).index(name), I=I)
        _TABLES[key] = (t, t.D @ t.D.t())
    return _TABLES[key]


def project_matrix(dtype):
    """An orthonormal U [r I, r I] (fp64 QR, rounded to ``dtype``), shared by every project case."""
    key = ("U", dtype)
    if key not in _TABLES:
        n = PROJECT_R * PROJECT_I
        _TABLES[key] = torch.linalg.qr(torch.randn(n, n, generator=torch.Generator().manual_seed(320), dtype=torch.float64)).Q.to(dtype)
    return _TABLES[key]


def project_table(name, dtype):
    """(Table, q, ref = D^T U[:, :q], scale = |D|^T |U[:, :q]|), built once."""
    key = ("project", name, dtype)
    if key not in _TABLES:
        cols, q = PROJECT_CASES[name]
        t = block_table(cols, PROJECT_R, dtype, 2000 + list(PROJECT_CASES).index(name), I=PROJECT_I)
        U = project_matrix(dtype).double()[:, :q]
        _TABLES[key] = (t, q, t.D.t() @ U, t.D.abs().t() @ U.abs())
    return _TABLES[key]


# ------------------------------------------------------------------------------------------------------------------- group
def group_reference(blk_i, I):
    """(ilist, iptr) as int64 arrays: the blocks whose index lies in [0, I) in a stable order by index, and the I + 1 offsets."""
    b = np.asarray(blk_i, dtype=np.int64)
    keep = np.nonzero((b >= 0) & (b < I))[0]
    ilist = keep[np.argsort(b[keep], kind="stable")]
    iptr = np.concatenate([[0], np.cumsum(np.bincount(b[keep], minlength=I))]).astype(np.int64)
    return ilist, iptr


GROUP_NB, GROUP_I = (0, 1, 255, 256, 257, 4096, 4097, 10000), (1, 257, 1000, 4096)
GROUP_BIG = (4200000, 3)  # group_chunk rises above 4096 blocks past 1024 * 4096 = 4,194,304 blocks


def group_input(nb, I, kind="random"):
    """int32 blk_i [nb]: ``random`` over [0, I); ``one_index`` all at I // 2; ``out_of_range`` with about a fifth of the entries
    equal to I or I + 1."""
    g = torch.Generator().manual_seed(7 * nb + I)
    if kind == "one_index":
        return torch.full((nb,), I // 2, dtype=torch.int32)
    b = torch.randint(0, I, (nb,), generator=g, dtype=torch.int32)
    if kind == "out_of_range":
        bad = torch.rand(nb, generator=g) < 0.2
        b[bad] = I + torch.randint(0, 2, (int(bad.sum()),), generator=g, dtype=torch.int32)
    return b


# --------------------------------------------------------------------------------------------------------- keys and levels
def keys_reference(X, shape):
    """key[p] = ((x_N I_{N-1} + x_{N-1}) ...) I_1 + x_1 in Python integers (x_N major, x_1 minor)."""
    keys = []
    for row in X.tolist():
        k = 0
        for n in range(len(shape) - 1, -1, -1):
            k = k * int(shape[n]) + int(row[n])
        keys.append(k)
    return keys


def levels_reference(Xsorted):
    """int32 [P]: the deepest mode (1-based) in which row p differs from row p - 1; N for p = 0; 0 for a repeated row."""
    Xs = np.asarray(Xsorted, dtype=np.int64)
    P, N = Xs.shape
    lev = np.full(P, N, dtype=np.int32)
    lev[1:] = ((Xs[1:] != Xs[:-1]) * np.arange(1, N + 1)).max(axis=1)
    return lev


KEYS_P = 600
KEYS_SHAPES = {1: [1000], 4: [7, 5, 9, 4]}
KEYS_BIG_SHAPE = [2**20, 2**21, 2**21]  # prod = 2^62: the largest key is 2^62 - 1


def keys_input(shape, seed, P=KEYS_P, corners=False):
    """int64 X [P, N], uniform over ``shape``; with ``corners`` its first 2^N rows are the corners (0 or I_n - 1 in every mode)."""
    g = torch.Generator().manual_seed(seed)
    X = torch.stack([torch.randint(0, int(s), (P,), generator=g, dtype=torch.int64) for s in shape], dim=1)
    if corners:
        for p, c in enumerate(itertools.product((0, 1), repeat=len(shape))):
            X[p] = torch.tensor([(int(s) - 1) * b for s, b in zip(shape, c)])
    return X


VALIDATE_P, VALIDATE_SHAPE = 270000, [5, 6, 7, 8]
# (flat element of X that is bad): the last one, and the first one of the grid-stride tail
VALIDATE_ELEMS = (VALIDATE_P * 4 - 1, VALIDATE_GRID_ELEMS)

LEVEL_EDGES = (255, 256, 257, 512)  # last thread of workgroup 0, first two of workgroup 1, first of workgroup 2


def sorted_set(levs, N, seed):
    """A strictly ascending sample set (x_N major) whose level sequence is ``levs`` (levs[0] must be N): sample p steps mode
    levs[p] and redraws the modes below it."""
    g = torch.Generator().manual_seed(seed)
    low = torch.randint(0, 3, (len(levs), N), generator=g).tolist()
    x, rows = [0] * N, []
    for p, l in enumerate(levs):
        if p > 0:
            x[l - 1] += 1
            x[: l - 1] = low[p][: l - 1]
        rows.append(list(x))
    return torch.tensor(rows, dtype=torch.int64)


def level_sequence(N, rotation, P=KEYS_P, seed=11):
    """Levels in 1..N, random except at LEVEL_EDGES, where edge k takes 1 + (k + rotation) mod N: over the N rotations every edge
    sees every level."""
    g = torch.Generator().manual_seed(seed + rotation)
    levs = torch.randint(1, N + 1, (P,), generator=g).tolist()
    levs[0] = N
    for k, p in enumerate(LEVEL_EDGES):
        levs[p] = 1 + (k + rotation) % N
    return levs


def shuffled(Xsorted, seed):
    """(X, perm int32) with X[perm] = Xsorted: the rows in a random order and the permutation that sorts them."""
    P = Xsorted.shape[0]
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(seed))
    X = torch.empty_like(Xsorted)
    X[perm] = Xsorted
    return X, perm.to(torch.int32)


# ------------------------------------------------------------------------------------------------------ sparse_canonical
# branch of _hipops.sparse_canonical -> (shape, samples).  [6, 5, 7, 4] has 840 cells: every one of them, shuffled; [60, 50, 70, 40]
# gives the int32 branch its 2000 samples.
CANONICAL_CASES = collections.OrderedDict([
    ("int32_all_cells", ([6, 5, 7, 4], 840)),
    ("int32", ([60, 50, 70, 40], 2000)),
    ("int64", ([2**12, 2**12, 2**12], 2000)),
    ("no_keys", ([2**22, 2**21, 2**21], 2000)),
])


def canonical_branch(shape):
    size = math.prod(int(s) for s in shape)
    return "int32" if size < 2**31 else "int64" if size < 2**63 else "no_keys"


def distinct_positions(shape, P, seed):
    """int64 [P, N] distinct positions in a random order: half drawn over the whole shape, half from the top 48 indices of
    every mode, and (when they fit) the all-zero and the all-maximal corner."""
    g = torch.Generator().manual_seed(seed)
    size = math.prod(int(s) for s in shape)
    if size <= P:
        assert size == P
        X = torch.stack(torch.unravel_index(torch.randperm(size, generator=g), shape), dim=1)
        return X.to(torch.int64).contiguous()
    seen, rows = set(), []

    def add(row):
        if row not in seen:
            seen.add(row)
            rows.append(row)

    add(tuple(0 for _ in shape))
    add(tuple(int(s) - 1 for s in shape))
    while len(rows) < P:
        lo = [0 if len(rows) % 2 == 0 else max(0, int(s) - 48) for s in shape]
        add(tuple(int(torch.randint(l, int(s), (1,), generator=g)) for l, s in zip(lo, shape)))
    X = torch.tensor(rows, dtype=torch.int64)
    return X[torch.randperm(P, generator=g)].contiguous()


# end to end: 300 samples, the full grid of a few index values per mode, of a rank-2 function, so that the tensor with zeros
# elsewhere has TT rank 2 and every unfolding stays inside the device envelope (rank x size <= 4096 rows in fp32, which rules the
# shapes of CANONICAL_CASES out: 2 x 4096 rows at their second bond).  branch -> (shape, grid sizes)
END_TO_END_CASES = collections.OrderedDict([
    ("int32", ([6, 5, 7, 4], (5, 4, 5, 3))),
    ("int64", ([64] * 6, (5, 5, 3, 2, 2, 1))),        # prod = 2^36
    ("no_keys", ([64] * 11, (5, 5, 3, 2, 2) + (1,) * 6)),  # prod = 2^66
])


def end_to_end_samples(name):
    """(X [300, N], y [300] fp64, Z [300, N]): the grid samples of f(x) = prod a_n(x_n) + prod b_n(x_n) in a random order, and 300
    held-out positions off the grid in one to three modes (the tensor is zero there).  Every mode's grid holds its last index."""
    shape, sizes = END_TO_END_CASES[name]
    g = torch.Generator().manual_seed(31 + len(shape))
    N = len(shape)
    grids, off = [], []
    for s, m in zip(shape, sizes):
        p = torch.randperm(s - 1, generator=g)
        grids.append(torch.cat([p[: m - 1], torch.tensor([s - 1])]).sort().values)
        off.append(p[m - 1 :])  # never empty: m < s in every case
    X = torch.cartesian_prod(*grids).reshape(-1, N)
    assert X.shape[0] == 300
    a = [0.5 + torch.rand(s, generator=g, dtype=torch.float64) for s in shape]
    b = [0.5 + torch.rand(s, generator=g, dtype=torch.float64) for s in shape]
    y = torch.stack([a[n][X[:, n]] for n in range(N)]).prod(0) + torch.stack([b[n][X[:, n]] for n in range(N)]).prod(0)
    order = torch.randperm(300, generator=g)
    Z = X[torch.randint(0, 300, (300,), generator=g)].clone()
    for p in range(300):
        for n in torch.randperm(N, generator=g)[: 1 + p % 3].tolist():
            Z[p, n] = off[n][int(torch.randint(0, len(off[n]), (1,), generator=g))]
    return X[order].contiguous(), y[order].contiguous(), Z


def evaluate(cores, X):
    """The train's values at the positions X, in fp64 on the CPU."""
    v = torch.ones(X.shape[0], 1, dtype=torch.float64)
    for n, c in enumerate(cores):
        v = torch.einsum("pa,apb->pb", v, c.detach().cpu().double()[:, X[:, n], :])
    return v[:, 0]

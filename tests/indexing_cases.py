"""Inputs, named cases and plain references for the point-evaluation kernels of ``tntorch_amd/csrc/ttr_index.hip`` (validate,
histogram, scan, scatter, gather, step), shared by tests/test_indexing_cases_host.py (which checks every reference here against
a brute-force loop, on the CPU) and tests/test_indexing_kernels_gpu.py.  Nothing here touches a device.

The constants mirror the kernel's documented geometry: a step tile is 64 rows by 64 columns with k staged in chunks of 32, the
histogram and the scatter keep up to 1024 bins in LDS, the scan walks the bins 1024 at a time, every per-point launch uses
workgroups of 256 threads, the gather grid stops at 65536 workgroups, and up to 1024 points skip the sort by default."""
import collections

import torch

TILE_ROWS, TILE_COLS, TILE_K, LDS_BINS, SCAN_CHUNK, THREADS = 64, 64, 32, 1024, 1024, 256
GATHER_GRID, DIRECT_MAX, MAX_RANK, MAX_BATCH = 65536, 1024, 512, 65535
SORTED, DIRECT, DEFAULT = 0, 1 << 40, -1  # direct_max_points that force either path, and the library's own choice
EPS = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}  # unit roundoff
INT_LIMIT = 2 ** 24  # integers up to here are exact in fp32 (and in fp64)


# -------------------------------------------------------------------------------------------------------------- references
def wrapped(col, I):
    """The index column as int64 on the CPU with negative entries wrapped as torch wraps them (-I <= i < I -> i mod I)."""
    c = col.detach().cpu().to(torch.int64)
    if c.numel() and (int(c.min()) < -I or int(c.max()) >= I):
        raise IndexError("index out of range for a mode of size {}".format(I))
    return torch.where(c < 0, c + I, c)


def chain_reference(cores, cols):
    """(ref, scale), both fp64 [B, r_0, P, r_N] on the CPU: ref[b, :, p, :] = G_a[b][:, i_a[p], :] @ ... @ G_z[b][:, i_z[p], :]
    for cores [B, r_n, I_n, r_{n+1}] and one index column per core, and scale the same chain over |G| (the elementwise sum of
    the absolute values of every product that enters an output: what a rounding error is relative to).  One index_select per
    mode and one batched matrix product per multiplied mode."""
    X = A = None
    for c, i in zip(cores, cols):
        G = c.detach().cpu().double()
        S = G.index_select(2, wrapped(i, G.shape[2])).permute(0, 2, 1, 3)  # [B, P, r, r']: one slice per point
        X, A = (S, S.abs()) if X is None else (torch.matmul(X, S), torch.matmul(A, S.abs()))
    return X.permute(0, 2, 1, 3).contiguous(), A.permute(0, 2, 1, 3).contiguous()


def brute_chain(cores, cols):
    """chain_reference's ref by Python loops over the batch, the points, the rows, the columns and k (tiny cases only)."""
    B, r0, P = cores[0].shape[0], cores[0].shape[1], cols[0].shape[0]
    out = torch.zeros(B, r0, P, cores[-1].shape[3], dtype=torch.float64)
    for b in range(B):
        for p in range(P):
            i = int(cols[0][p])
            M = [[float(cores[0][b, a, i, j]) for j in range(cores[0].shape[3])] for a in range(r0)]
            for c, col in zip(cores[1:], cols[1:]):
                i = int(col[p])  # a negative Python index wraps as torch's does
                M = [[sum(M[a][k] * float(c[b, k, i, j]) for k in range(c.shape[1])) for j in range(c.shape[3])] for a in range(r0)]
            out[b, :, p, :] = torch.tensor(M, dtype=torch.float64)
    return out


def error_bound(ranks, dtype, scale):
    """|out - ref| <= 2 (sum over the multiplied modes of (r_n + 2)) u scale, elementwise: the bound of one gather step
    (test_cross_kernels_gpu.check_gather: an FMA chain of length r_n, 2 (r_n + 2) u) carried over the chain, the errors of
    successive modes compounding to first order.  The first mode is a copy.  A one-mode chain has the bound 0."""
    return 2 * sum(r + 2 for r in ranks[1:-1]) * EPS[dtype] * scale


def int_bound(ranks):
    """|x| <= 2^N prod(inner ranks) for every output and every partial sum of a chain over int_cores: an entry is at most 2 in
    magnitude, so after mode n every |X| entry, and every partial sum of the FMA chain that forms it, is at most
    2^(n+1) r_1 ... r_n, which grows with n."""
    b = 2 ** (len(ranks) - 1)
    for r in ranks[1:-1]:
        b *= r
    return b


def int_cores(ranks, sizes, B, seed):
    """fp64 cores [B, r_n, I_n, r_{n+1}] with integer entries drawn from {-2, ..., 2}, different for every batch item.  The
    ranks must keep int_bound(ranks) far below 2^24 (asserted: at most 2^20): then every product and every partial sum is an
    integer that fp32 holds exactly, the device result is exact in fp32 and in fp64 whatever the summation order, and a point
    routed to the wrong group, slice or output row changes an integer."""
    assert int_bound(ranks) <= 2 ** 20 < INT_LIMIT, (ranks, int_bound(ranks))
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(-2, 3, (B, ranks[n], int(sizes[n]), ranks[n + 1]), generator=g).double() for n in range(len(sizes))]


def gauss_cores(ranks, sizes, B, seed, dtype):
    """Gaussian cores scaled by r_n^-1/2, rounded to ``dtype`` (the reference then runs on the rounded values)."""
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(B, ranks[n], int(sizes[n]), ranks[n + 1], generator=g, dtype=torch.float64) / ranks[n] ** 0.5).to(dtype)
            for n in range(len(sizes))]


def random_cols(sizes, P, seed, negative=True):
    """One int64 column per mode, uniform over [-I, I) (negative entries wrap) or over [0, I)."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(-int(I) if negative else 0, int(I), (P,), generator=g) for I in sizes]


def counts_column(counts, seed):
    """A shuffled int64 index column in which value v occurs exactly counts[v] times."""
    col = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(list(counts), dtype=torch.int64))
    return col[torch.randperm(col.numel(), generator=torch.Generator().manual_seed(seed))].contiguous()


# ------------------------------------------------------------------------------------------------------------------- cases
# Integer-core families of the GPU file: name -> (ranks, sizes, B).  int_bound of each is checked on the CPU.
BINS_RANKS, BINS_I, BINS_P = [2, 3, 3, 2], (1023, 1024, 1025, 2047, 2048, 2049, 3000), (5000, 300)
CHANGING_RANKS, CHANGING_SIZES, CHANGING_LARGER, CHANGING_P = [2, 3, 2, 3, 2, 2], [5, 2049, 3, 1025, 1], [5, 4000, 3000, 2500, 3000], 2500
LEAD_RA, LEAD_I, LEAD_P, LEAD_B = (1, 3, 63, 64, 65, 128, 130, 512), 3, 37, 2
TILE_EDGE_COUNTS = collections.OrderedDict([(1, (0, 64, 0, 65, 1, 63, 0, 128)), (3, (21, 22, 43, 0, 1, 64)), (65, (1, 0, 64, 63))])
SWITCH_P, SWITCH_SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025), [4, 1030, 6]
FORMS_P, FORMS_SIZES = 3000, [5, 7, 1500]
OOB_I, OOB_RANKS = (6, 1500), [2, 3, 3, 2]
ONE_MODE = [(1, 1, 1, 1, 1), (17, 3, 5, 7, 2), (300, 1, 1, 2000, 1), (1025, 65, 3, 4, 2), (257, 2, 130, 3, 1)]  # P, ra, rn, I, B
ONE_MODE_BIG = (66000, 4, 64, 5, 1)  # P ra rn = 16,896,000 > 65536 * 256 = 16,777,216: the grid-stride loop's second trip
API_SHAPE, API_RANKS, API_P = [4, 6, 1500, 5], [1, 65, 65, 7, 1], 2000


def lead_ranks(ra, gauss=False):
    return [ra, 33, 65, 70] if gauss else [ra, 33, 3, 2]


INT_CASES = collections.OrderedDict()
for _I in BINS_I:
    INT_CASES["bins_{}".format(_I)] = (BINS_RANKS, [7, _I, _I], 1)
INT_CASES["changing"] = (CHANGING_RANKS, CHANGING_SIZES, 2)
INT_CASES["changing_larger"] = (CHANGING_RANKS, CHANGING_LARGER, 2)
for _ra in LEAD_RA:
    INT_CASES["lead_{}".format(_ra)] = (lead_ranks(_ra), [LEAD_I] * 3, LEAD_B)
for _ra, _counts in TILE_EDGE_COUNTS.items():
    INT_CASES["tile_edges_{}".format(_ra)] = ([_ra, 3, 3, 2], [4, len(_counts), len(_counts)], 2)
INT_CASES["switch"] = ([2, 3, 3, 2], SWITCH_SIZES, 2)
INT_CASES["forms"] = ([2, 3, 3, 2], FORMS_SIZES, 2)
INT_CASES["strides_1"] = ([3, 5], [1030], 2)
INT_CASES["strides_3"] = ([3, 5, 4, 5], [6, 1030, 5], 2)
for _I in OOB_I:
    INT_CASES["oob_{}".format(_I)] = (OOB_RANKS, [_I + 2] * 3, 1)  # allocated with one spare slice on each side
INT_CASES["batch_limit"] = ([1, 1, 1], [1, 1], MAX_BATCH)
INT_CASES["workspace"] = ([2, 3, 3, 2], [5, 1030, 6], 1)

_CORES, _REFS = {}, {}


def case_cores(name):
    """The fp64 integer cores of INT_CASES[name], built once."""
    if name not in _CORES:
        ranks, sizes, B = INT_CASES[name]
        _CORES[name] = int_cores(ranks, sizes, B, 4000 + list(INT_CASES).index(name))
    return _CORES[name]


def cached_reference(key, cores, cols):
    """chain_reference(cores, cols)[0], computed once per ``key`` (fp32 and fp64 runs of an integer case share it)."""
    if key not in _REFS:
        _REFS[key] = chain_reference(cores, cols)[0]
    return _REFS[key]

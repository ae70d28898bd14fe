"""Truths, error bounds and kernel shapes the host and the GPU tests of ``tn.tt_lookup`` / ``ttr_ttm_lookup_step`` share.

The reference has no row lookup, so there is no recorded output: the truth is the dense fp64 matrix of ``matrix_cases.tt_dense``
(a plain contraction, independent of the package) indexed with the rows.  The bounds are ``matrix_cases``' with ``x`` one-hot
(u = 2^-24 in fp32, 2^-53 in fp64; |.| elementwise):
    one step   |Y - Y64| <= 2 (R + 1) u (|X| . |G|)                  a dot product of R terms and the cast of the result
    the chain  |y - y64| <= 2 (sum_k r_{k-1} + d) u |M|[rows]        |M| = the matrix of the cores' magnitudes
(the relative errors of chained steps multiply, (1 + gamma_a)(1 + gamma_b) <= 1 + gamma_{a + b}, for any order of the sums)."""
import torch

import matrix_cases as mc
import tntorch_amd as tn

# ttr_ttm_lookup_step: (P, D, R, I, O, S).  R in {1, 3, 4, 33}: fewer than 4 r, a quad that straddles R, more than one chunk
# of 32; D in {1, 3, 17, 65}: a sample's rows split across tiles of 64, more rows than a tile; O S in {1, 15, 64, 80}: less
# than a column tile of 16, a whole tile of 64, a second one; I in {1, 5, 1025}: 1025 is beyond the LDS histogram bins;
# P in {1, 63, 64, 65, 300}.  Every value of each axis occurs.
STEP_SHAPES = [
    (1, 1, 1, 1, 1, 1), (63, 3, 3, 5, 3, 5), (64, 17, 4, 5, 8, 8), (65, 65, 33, 5, 5, 16), (300, 1, 4, 1025, 1, 1),
    (300, 3, 33, 5, 15, 1), (64, 1, 3, 1, 16, 5), (65, 17, 1, 1025, 3, 5), (1, 65, 4, 5, 64, 1), (63, 1, 33, 1025, 4, 16),
    (300, 17, 3, 5, 1, 1), (65, 3, 1, 1, 8, 8),
]


def lookup_rows(rows_total):
    """Rows with duplicates, negatives and both ends of the range, [2, 6]."""
    g = torch.Generator().manual_seed(11)
    r = torch.randint(-rows_total, rows_total, (2, 6), generator=g)
    r[0, 0], r[0, 1], r[1, 0], r[1, 1], r[1, 2] = 0, rows_total - 1, -rows_total, -1, r[0, 2]
    return r


def truth_and_bound(cores, rows, dtype):
    """(y64, bound) of ``tt_lookup``: the rows of the dense fp64 matrix of the cores as given (cast), and the chain bound."""
    M = mc.tt_dense(cores)
    # the digit order: i_1 most significant, as TTMatrix.torch() has it (the matrices of these tests are tiny)
    idims, odims = [c.shape[1] for c in cores], [c.shape[2] for c in cores]
    T = tn.TTMatrix([c.detach().double().cpu() for c in cores], None, idims, odims).torch()
    assert T.shape == M.shape and torch.allclose(T, M, rtol=1e-12, atol=1e-12 * float(M.abs().max()))
    rows = torch.as_tensor(rows).cpu().long()
    mag = mc.tt_dense([c.abs() for c in cores])
    n = sum(int(c.shape[0]) for c in cores) + len(cores)
    return M[rows], 2 * n * mc.unit(dtype) * mag[rows]


def step_operands(shape, dtype, seed=5, rows_x=None):
    """X [rows_x or P, D, R], G [R, I, O, S] (drawn in fp64 and cast) and idx [P] in [-I, I) (int64)."""
    P, D, R, I, O, S = shape
    g = torch.Generator().manual_seed(seed)
    X = torch.randn((rows_x or P, D, R), dtype=torch.float64, generator=g).to(dtype)
    G = torch.randn((R, I, O, S), dtype=torch.float64, generator=g).to(dtype)
    idx = torch.randint(-I, I, (P,), generator=g)
    return X, G, idx


def step_truth_and_bound(X, xrow, G, idx, dtype):
    """The einsum of the contract in fp64 on the CPU, and 2 (R + 1) u times the einsum of the magnitudes."""
    X, G = X.detach().double().cpu(), G.detach().double().cpu()
    idx = idx.cpu().long()
    Xg = X if xrow is None else X[xrow.cpu().long()]
    Gg = G[:, torch.where(idx < 0, idx + G.shape[1], idx)]
    Y = torch.einsum("pdr,rpos->pdos", Xg, Gg)
    mag = torch.einsum("pdr,rpos->pdos", Xg.abs(), Gg.abs())
    return Y, 2 * (X.shape[2] + 1) * mc.unit(dtype) * mag

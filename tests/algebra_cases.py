"""The shapes, operands, fp64 truths and error bounds the host and the GPU tests of ``tn.tt_apply`` / ``tn.tt_matmul`` /
``tn.tt_transpose`` and of the kernel behind them, ``ttr_core_compose``, share.

    compose(A, B)[r S1 + a, p, q, s S2 + b] = sum_j A[r, p, j, s] B[a, j, q, b],    A [R1, P, J, R2], B [S1, J, Q, S2]

The bounds are derived, not tuned, as in matrix_cases.py (u = 2^-24 in fp32, 2^-53 in fp64; |.| elementwise):
    one core        |out - out64| <= 2 (J + 1) u (|A| o |B|)            the same einsum on the absolute values
    a whole product |y - y64| <= 2 n u mag,  n = sum_k (J_k + R_k S_k) + 2 d
for any order of the sums: a dot product of n terms is off by at most gamma_n <= 2 n u / 1.9 times the product of the absolute
values, and chained relative errors add up in the index of gamma.  n counts the compose chain of every core (J_k terms), the
chain of the decompression GEMM over the merged rank that enters core k (R_k S_k terms) and two roundings of stored values per
mode (the core and the running dense product).  mag is the same product built from the absolute values of the cores.  The truth
is an fp64 CPU contraction of the operands as given (cast), independent of the package (``mc.tt_dense``, ``train_dense``)."""
import numpy as np
import torch

import matrix_cases as mc
from tntorch_amd import _hip

unit = mc.unit
TILE_M, TILE_N, TILE_K = _hip.COMPOSE_TILE_M, _hip.COMPOSE_TILE_N, _hip.COMPOSE_TILE_K

# (R1, P, J, R2, S1, Q, S2)
BASE_SHAPES = [
    (1, 1, 1, 1, 1, 1, 1),        # all extents 1
    (1, 1, 4, 3, 5, 7, 1),        # first core of t @ M
    (3, 1, 5, 2, 4, 6, 5),        # middle core of t @ M; J is no multiple of 4
    (4, 6, 5, 5, 3, 1, 2),        # M @ u, Q = 1
    (2, 3, 3, 4, 3, 2, 5),        # general, J < 4
    (7, 1, 33, 5, 2, 3, 17),      # J across a staging chunk; odd run length
    (16, 2, 2, 16, 16, 2, 16),    # powers of two; pack path; run of 256; 8 x 8 tiles
    (1, 5, 7, 1, 1, 4, 1),        # rank 1 on both sides; run of length 1
    (5, 1, 4, 13, 3, 1, 5),       # run of 65
    (33, 1, 2, 3, 2, 1, 33),      # many short rows
    (3, 5, 70, 9, 4, 3, 7),       # three chunks of j; 135 rows x 84 columns: partial tiles on both sides
    (2, 1, 6, 3, 1, 2, 80),       # S2 above the column tile: a run cut by tiles, a segment boundary inside a tile
]


def _pair(v):
    """v = x y with x <= y as close as they get (a prime: 1 x v)"""
    x = max(d for d in range(1, int(v ** 0.5) + 1) if v % d == 0)
    return x, v // x


def _edge_shapes():
    """R1 P R2, S1 Q S2 and R2 S2 at every tile extent minus 1, exactly at it and plus 1"""
    out = []
    for ext in sorted({TILE_M, TILE_N, TILE_K}):
        for v in (ext - 1, ext, ext + 1):
            x, y = _pair(v)
            out.append((v, 1, 5, 1, 2, 3, 2))          # rows = v through R1
            out.append((x, y, 3, 1, 3, 1, 4))          # rows = v through R1 P
            out.append((2, 3, 5, 2, v, 1, 1))          # columns = v through S1
            out.append((3, 1, 6, 4, 1, x, y))          # columns = v through Q S2
            out.append((1, 2, 3, v, 2, 1, 1))          # run = v through R2
            out.append((2, 1, 3, x, 1, 2, y))          # run = v through R2 S2
            out.append((1, 1, 2, 1, 2, 3, v))          # run = v through S2
    return out


SHAPES = list(dict.fromkeys(BASE_SHAPES + _edge_shapes()))
assert all(s[0] * s[4] * s[1] * s[5] * s[3] * s[6] < 1_000_000 for s in SHAPES)
assert all(any(s[ax] == 1 for s in SHAPES) for ax in range(7))


def operands(shape, dtype, seed=5):
    R1, P, J, R2, S1, Q, S2 = shape
    g = torch.Generator().manual_seed(seed)
    A = torch.randn((R1, P, J, R2), dtype=torch.float64, generator=g).to(dtype)
    B = torch.randn((S1, J, Q, S2), dtype=torch.float64, generator=g).to(dtype)
    return A, B


def compose64(A, B):
    A, B = A.detach().double().cpu(), B.detach().double().cpu()
    R1, P, _, R2 = A.shape
    S1, _, Q, S2 = B.shape
    return torch.einsum("rpjs,ajqb->rapqsb", A, B).reshape(R1 * S1, P, Q, R2 * S2)


def core_truth_and_bound(A, B, dtype):
    """(out64, bound) of one core from the operands as given (cast)."""
    return compose64(A, B), 2 * (A.shape[2] + 1) * unit(dtype) * compose64(A.abs(), B.abs())


# ------------------------------------------------------------------ whole products
TRAIN_RANKS = {"ref": [4], "three": [3, 2], "single": [], "kron": [2, 3]}
CASES = list(mc.RANDOM_CASES)


def train_cores(dims, ranks, dtype, seed=11):
    g = torch.Generator().manual_seed(seed)
    rk = [1] + list(ranks) + [1]
    return [torch.randn((rk[k], int(n), rk[k + 1]), dtype=torch.float64, generator=g).to(dtype) for k, n in enumerate(dims)]


def case(name, dtype):
    """(matrix cores G, a train over input_dims T, a train over output_dims U, input_dims, output_dims) of a case."""
    idims, odims = mc.RANDOM_CASES[name][:2]
    G = mc.random_cores(name, dtype)[0]
    return G, train_cores(idims, TRAIN_RANKS[name], dtype, 11), train_cores(odims, TRAIN_RANKS[name], dtype, 12), idims, odims


def train_dense(cores):
    """The dense tensor of TT cores [a, n, b], flattened, in fp64 on the CPU, by plain contraction."""
    acc = None
    for c in cores:
        c = c.detach().double().cpu()
        acc = c if acc is None else torch.einsum("anb,bmc->anmc", acc, c).reshape(acc.shape[0], -1, c.shape[2])
    return acc[0, :, 0]


def _chain_terms(pairs):
    """n = sum_k (J_k + R_k S_k) + 2 d for the (first core, second core, J) of every mode"""
    return sum(J + int(x.shape[0]) * int(y.shape[0]) for x, y, J in pairs) + 2 * len(pairs)


def apply_truth_and_bound(G, T, dtype, transpose=False):
    """(y64, bound), flat: vec(t) @ M, or M @ vec(t) for ``transpose``."""
    M, Mabs = mc.tt_dense(G), mc.tt_dense([g.abs() for g in G])
    v, vabs = train_dense(T), train_dense([c.abs() for c in T])
    n = _chain_terms([(g, c, int(c.shape[1])) for g, c in zip(G, T)])
    if transpose:
        return M @ v, 2 * n * unit(dtype) * (Mabs @ vabs)
    return v @ M, 2 * n * unit(dtype) * (vabs @ Mabs)


def matmul_truth_and_bound(GA, GB, dtype):
    n = _chain_terms([(a, b, int(a.shape[2])) for a, b in zip(GA, GB)])
    return mc.tt_dense(GA) @ mc.tt_dense(GB), 2 * n * unit(dtype) * (mc.tt_dense([g.abs() for g in GA]) @ mc.tt_dense([g.abs() for g in GB]))


def transposed(G):
    return [g.permute(0, 2, 1, 3) for g in G]


def rel_err(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return float(np.linalg.norm(x - y) / np.linalg.norm(y))

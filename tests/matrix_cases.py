"""The cases of tests/golden/matrix_f64.npz (tools/gen_matrix_golden.py), the shapes of the kernel tests and the error bounds the
host and the GPU tests of ``tn.tt_multiply`` / ``tn.cp_multiply`` share.

A golden case is a random fp64 matrix drawn after ``torch.manual_seed(SEED)``; the fixture holds the matrix (``<case>_M``), the
cores of the reference's ``TTMatrix(M, ranks, ...)`` (``<case>_tt<k>``) and ``CPMatrix(M, cp_rank, ...)`` (``<case>_cp<k>``) as
the reference built them, the input (``<case>_x``) and the reference's ``tt_multiply`` / ``cp_multiply`` outputs (``<case>_tty``,
``<case>_cpy``).

The bounds are derived, not tuned (u = 2^-24 in fp32, 2^-53 in fp64; |.| elementwise):
    one step   |Y - Y64| <= 2 (K + 1) u (|X| . |G|),                              K = I R (tt) or I (cp)
    a chain    |y - y64| <= 2 (sum_k K_k + d) u (|x| . |G_0| ... |G_{d-1}|)       cp: + R for the final sum over the rank
for any order of the sums: a dot product of n terms in floating point is off by at most gamma_n = n u / (1 - n u) <= 2 n u / 1.9
times the product of the absolute values, the relative errors of chained steps multiply, (1 + gamma_a)(1 + gamma_b) <=
1 + gamma_{a + b}, and the cast of the result (the truth is compared after the operands were cast, so only the d stored
intermediates round) adds one u per step.  Against outputs the reference recorded in fp64 the bound is doubled: its own rounding
obeys the same bound."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 7
# name -> (input_dims, output_dims, tt ranks, cp rank, batch)
CASES = {
    "ref": ([11, 3], [23, 2], [50], 5, 30),          # the shapes of the reference's tests/test_matrix.py
    "three": ([4, 3, 5], [2, 6, 3], [7, 5], 4, 9),
}
# host / device products from cores drawn here (not recorded): name -> (input_dims, output_dims, tt ranks, cp rank, batch)
RANDOM_CASES = {
    "ref": ([11, 3], [23, 2], [50], 50, 30),
    "three": ([4, 3, 5], [2, 6, 3], [7, 5], 6, 9),
    "single": ([5], [7], [], 3, 4),
    "kron": ([3, 4, 2], [2, 5, 3], [1, 1], 1, 5),
}

# ttr_ttm_step: (I, D, R, O, S).  D in {1, 15, 17, 129, 257}; (I, R) in {(1, 1), (4, 1), (2, 3), (7, 5), (3, 16), (2, 33)}: K < 4,
# quads of k that straddle two i (R = 3, 5, 33), K across tiles of 32 (35, 48, 66); (O, S) in {(1, 1), (3, 1), (4, 4), (1, 17),
# (5, 26)}: N < 16, N = 16, N across tiles of 64 (130).  Every value of each axis occurs, with each of the others' extremes.
TTM_SHAPES = [
    (1, 1, 1, 1, 1), (4, 15, 1, 3, 1), (2, 17, 3, 4, 4), (7, 129, 5, 1, 17), (3, 257, 16, 5, 26), (2, 129, 33, 3, 1),
    (2, 1, 33, 5, 26), (1, 257, 1, 4, 4), (7, 15, 5, 5, 26), (3, 17, 16, 1, 1), (4, 129, 1, 1, 17), (2, 257, 3, 3, 1),
    (7, 17, 5, 4, 4), (3, 15, 16, 1, 17), (2, 15, 33, 4, 4),
]
TTM_BIG = (5, 150, 20, 9, 16)   # M = 150 (3 tiles of 64), N = 144 (3 tiles), K = 100 (4 tiles of 32, R no power of two)
TTM_BIG_P2 = (4, 130, 32, 5, 16)   # the power-of-two instance: K = 128 (4 tiles), N = 80, M = 130
# ttr_cpm_step: (I, D, O, R); R in {1, 3, 4, 50}, D in {1, 63, 65, 1025}
CPM_SHAPES = [(1, 1, 1, 1), (3, 63, 2, 3), (5, 65, 3, 4), (2, 1025, 2, 50), (4, 1025, 1, 1), (3, 1, 4, 50), (2, 63, 5, 4), (6, 65, 1, 3),
              (3, 1025, 3, 4)]

_Z = None


def unit(dtype):
    return 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53


def fixture():
    global _Z
    if _Z is None:
        with np.load(os.path.join(ROOT, "tests", "golden", "matrix_f64.npz")) as z:
            _Z = {k: z[k] for k in z.files}
    return _Z


def draw_matrix(name):
    """The matrix and the input of a golden case, as the recording tool draws them."""
    idims, odims, _, _, b = CASES[name]
    g = torch.Generator().manual_seed(SEED)
    rows, cols = int(np.prod(idims)), int(np.prod(odims))
    M = torch.rand((rows, cols), dtype=torch.float64, generator=g)
    x = torch.randn((b, rows), dtype=torch.float64, generator=g)
    return M, x


def golden(name, dtype=torch.float64, device="cpu"):
    """dict(M, x, tt (cores), cp (cores), tty, cpy) of a golden case; the operands cast to ``dtype`` on ``device``, the recorded
    outputs left in fp64 on the CPU."""
    z, d = fixture(), len(CASES[name][0])
    conv = lambda a: torch.from_numpy(a).to(dtype).to(device)
    return dict(M=conv(z[name + "_M"]), x=conv(z[name + "_x"]), tt=[conv(z[f"{name}_tt{k}"]) for k in range(d)],
                cp=[conv(z[f"{name}_cp{k}"]) for k in range(d)], tty=torch.from_numpy(z[name + "_tty"]),
                cpy=torch.from_numpy(z[name + "_cpy"]))


def random_cores(name, dtype, seed=3):
    """(tt cores [r, I, O, r'], cp cores [I, O, R], x [b, rows]) of a RANDOM_CASES entry, drawn in fp64 and cast.  The tt ranks are
    taken as given (not capped by the mode sizes: the product does not care)."""
    idims, odims, ranks, R, b = RANDOM_CASES[name]
    g = torch.Generator().manual_seed(seed)
    rk = [1] + list(ranks) + [1]
    tt = [torch.randn((rk[k], idims[k], odims[k], rk[k + 1]), dtype=torch.float64, generator=g).to(dtype) for k in range(len(idims))]
    cp = [torch.randn((idims[k], odims[k], R), dtype=torch.float64, generator=g).to(dtype) for k in range(len(idims))]
    x = torch.randn((b, int(np.prod(idims))), dtype=torch.float64, generator=g).to(dtype)
    return tt, cp, x


def tt_dense(cores):
    """The dense [rows, cols] matrix of TT-matrix cores, in fp64 on the CPU, by plain contraction (independent of the package)."""
    acc = None
    for G in cores:
        G = G.detach().double().cpu()
        acc = G if acc is None else torch.einsum("aiob,bjpc->aijopc", acc, G).reshape(acc.shape[0], acc.shape[1] * G.shape[1],
                                                                                       acc.shape[2] * G.shape[2], G.shape[3])
    return acc[0, :, :, 0]


def cp_dense(cores):
    acc = None
    for C in cores:
        C = C.detach().double().cpu()
        acc = C if acc is None else torch.einsum("ior,jpr->ijopr", acc, C).reshape(acc.shape[0] * C.shape[0], acc.shape[1] * C.shape[1],
                                                                                    C.shape[2])
    return acc.sum(dim=-1)


def tt_truth_and_bound(cores, x2d, dtype, doubled=False):
    """(y64, bound): x2d @ M in fp64 on the CPU from the operands as given (cast), and the chain bound elementwise."""
    x = x2d.detach().double().cpu().reshape(-1, tt_dense(cores).shape[0])
    y64 = x @ tt_dense(cores)
    mag = x.abs() @ tt_dense([c.abs() for c in cores])
    n = sum(int(c.shape[0]) * int(c.shape[1]) for c in cores) + len(cores)
    return y64, (4 if doubled else 2) * n * unit(dtype) * mag


def cp_truth_and_bound(cores, x2d, dtype, doubled=False):
    x = x2d.detach().double().cpu().reshape(-1, cp_dense(cores).shape[0])
    y64 = x @ cp_dense(cores)
    mag = x.abs() @ cp_dense([c.abs() for c in cores])
    n = sum(int(c.shape[0]) for c in cores) + int(cores[0].shape[2]) + len(cores)
    return y64, (4 if doubled else 2) * n * unit(dtype) * mag


def assert_within(y, y64, bound, what=""):
    y = y.detach().double().cpu()
    assert y.shape == y64.shape, (what, y.shape, y64.shape)
    err = (y - y64).abs()
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print("{}: largest error / bound = {:.3f}".format(what, worst))
    assert bool((err <= bound).all()), "{}: error reaches {:.3f} of the bound".format(what, worst)


# ------------------------------------------------------------------ one step
def ttm_operands(shape, dtype, seed=1):
    I, D, R, O, S = shape
    g = torch.Generator().manual_seed(seed)
    X = torch.randn((I, D, R), dtype=torch.float64, generator=g).to(dtype)
    G = torch.randn((R, I, O, S), dtype=torch.float64, generator=g).to(dtype)
    return X, G


def ttm_truth_and_bound(X, G, dtype):
    X, G = X.detach().double().cpu(), G.detach().double().cpu()
    Y = torch.einsum("idr,rios->dos", X, G)
    mag = torch.einsum("idr,rios->dos", X.abs(), G.abs())
    return Y, 2 * (X.shape[0] * X.shape[2] + 1) * unit(dtype) * mag


def cpm_operands(shape, dtype, x_has_rank, seed=2):
    I, D, O, R = shape
    g = torch.Generator().manual_seed(seed)
    X = torch.randn((I, D, R) if x_has_rank else (I, D), dtype=torch.float64, generator=g).to(dtype)
    C = torch.randn((I, O, R), dtype=torch.float64, generator=g).to(dtype)
    return X, C


def cpm_truth_and_bound(X, C, dtype):
    X, C = X.detach().double().cpu(), C.detach().double().cpu()
    if X.dim() == 2:
        X = X[:, :, None]
    Y = torch.einsum("idr,ior->dor", X.expand(-1, -1, C.shape[2]), C)
    mag = torch.einsum("idr,ior->dor", X.abs().expand(-1, -1, C.shape[2]), C.abs())
    return Y, 2 * (X.shape[0] + 1) * unit(dtype) * mag

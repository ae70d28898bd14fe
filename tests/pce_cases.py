"""Cases, truths and bounds of the PCE tests (``PCEInterpolator``, ``ttr_pce_design`` / ``ttr_pce_predict``, ``_lars``), shared by
tests/test_pce_host.py, tests/test_pce_kernels_gpu.py and tests/test_pce_gpu.py.

Definitions: Z [P, N] the centred features, Psi [N, S, S], coords [C, N];  B(p, n, s) = sum_k Z[p, n]^k Psi[n, k, s];
design M[p, c] = prod_n B(p, n, coords[c, n]);  predict y[p] = sum_c coef[c] M[p, c].
"""
import functools
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pce_f64.npz")

# ---------------------------------------------------------------------------------------------- the kernels' grid
KERNEL_P = (1, 63, 64, 65, 257, 1000)
KERNEL_C = (1, 19, 64, 65, 300)
KERNEL_NS = ((1, 1), (3, 4), (5, 3))
EXTRA_PC = ((65, 19), (257, 300))    # the two (P, C) pairs of the grid for the further (N, S)
HOST_SHAPES = ((1, 1, 1, 1), (7, 1, 4, 4), (33, 3, 4, 19), (20, 5, 3, 21), (9, 2, 8, 30))   # (P, N, S, C)

# ---------------------------------------------------------------------------------------------- tolerances against the fixture
# Measured on the CPU mirror against tests/golden/pce_f64.npz (relative 2-norm deviations): coef 5.6e-16, predictions 5.7e-16,
# the dense tensor of to_tensor(domain=8, eps=1e-10) 6.2e-14.  Allowed: 100 x that (the cap of 1e-8 is not reached).
FIXTURE_COEF_TOL = 5.6e-14
FIXTURE_PREDICT_TOL = 5.7e-14
FIXTURE_DENSE_TOL = 6.2e-12
# LARS against scikit-learn, relative to the path's largest entry, with an fp64 / fp32 Gram matrix
LARS_TOL_F64, LARS_TOL_F32 = 1e-12, 1e-5
LARS_PROBLEMS = ((300, 3, 4), (500, 4, 3), (200, 2, 5), (257, 5, 3))   # (P, N, p), noise 0.3
RECOVERY_TOL = 1e-10          # fit + predict on the exactly representable polynomial, fp64
TENSOR_TOL = 1e-8             # to_tensor(eps=1e-10) against predict on the grid, relative to ||predict||
GPU_F32_PREDICT_CAP = 1e-4    # fp32 device prediction against the CPU mirror's fp64 one

_Z = None


def fixture():
    global _Z
    if _Z is None:
        with np.load(GOLDEN) as z:
            _Z = {k: z[k] for k in z.files}
    return _Z


# ---------------------------------------------------------------------------------------------- truths
def loops_design(Z, Psi, coords):
    """The definition with explicit loops, in fp64 (power sums, not Horner): M [P, C] as a NumPy array."""
    Z, Psi, coords = np.asarray(Z, dtype=np.float64), np.asarray(Psi, dtype=np.float64), np.asarray(coords)
    P, N = Z.shape
    S, C = Psi.shape[1], coords.shape[0]
    M = np.ones((P, C))
    for p in range(P):
        for c in range(C):
            for n in range(N):
                b = 0.0
                for k in range(S):
                    b += Z[p, n] ** k * Psi[n, k, coords[c, n]]
                M[p, c] *= b
    return M


def truth_design(Z, Psi, coords):
    """(M, A): the definition in fp64 (vectorised power sums) and the same expression on absolute values, NumPy [P, C]."""
    Z, Psi, coords = np.asarray(Z, dtype=np.float64), np.asarray(Psi, dtype=np.float64), np.asarray(coords)
    S = Psi.shape[1]
    V = Z[:, :, None] ** np.arange(S)                      # [P, N, S(k)]
    B = np.einsum("pnk,nks->pns", V, Psi)
    Ba = np.einsum("pnk,nks->pns", np.abs(V), np.abs(Psi))
    M, A = np.ones((Z.shape[0], coords.shape[0])), np.ones((Z.shape[0], coords.shape[0]))
    for n in range(Z.shape[1]):
        M *= B[:, n, coords[:, n]]
        A *= Ba[:, n, coords[:, n]]
    return M, A


def kernel_bound(N, S, Cp, dt, truth, A):
    """Entry-wise bound of the kernels (and of the CPU mirrors) against the fp64 truth: ``(2 S + N + C' + 4) 2^-52 A``, plus
    ``2^-23 |truth|`` in fp32.  A basis value by Horner in fp64 carries a relative error of at most 2 S u of its absolute sum
    (S - 1 FMAs, the conversion of the operands is exact), the truth's own power sum as much again: together within 2 S 2^-52;
    the product over N modes adds N u, the sum over C' candidates (C' = 0 for the design matrix, C for predict) C' u -- one FMA
    each -- and 4 u cover the truth's own roundings of the product and the sum.  ``A`` is the same expression on absolute
    values.  The single rounding to fp32 at the store is 2^-24 |value|, written 2^-23 |truth|."""
    bound = (2 * S + N + Cp + 4) * 2.0 ** -52 * A
    if dt == torch.float32:
        bound = bound + 2.0 ** -23 * np.abs(truth)
    return bound


@functools.lru_cache(maxsize=None)
def kernel_inputs(N, S, dt, P=max(KERNEL_P), C=max(KERNEL_C), seed=0):
    """(Z [P, N], Psi [N, S, S], coords [C, N], coef [C]) as CPU tensors of ``dt`` (coords int64) and the truths (M, A) of
    the design matrix on them.  Sub-cases take leading rows of Z and of coords / coef."""
    g = torch.Generator().manual_seed(1000 * N + 10 * S + seed)
    half = 1.5 if S <= 4 else 1.0    # (powers up to 15 of a wider range leave fp32 in a product over 16 modes)
    Z = ((torch.rand(P, N, generator=g, dtype=torch.float64) * 2.0 - 1.0) * half).to(dt)
    Psi = (torch.triu(torch.randn(N, S, S, generator=g, dtype=torch.float64)) * 0.5 + torch.eye(S, dtype=torch.float64)).to(dt)
    coords = torch.randint(0, S, (C, N), generator=g)
    coef = torch.randn(C, generator=g, dtype=torch.float64).to(dt)
    M, A = truth_design(Z.double().numpy(), Psi.double().numpy(), coords.numpy())
    return Z, Psi, coords, coef, M, A


def truth_predict(M, A, coef, P, C):
    """(y, Ay) for the leading P points and C candidates from the design truths."""
    cf = coef[:C].double().numpy()
    return M[:P, :C] @ cf, A[:P, :C] @ np.abs(cf)


# ---------------------------------------------------------------------------------------------- regression problems
def recovery_problem(dt=torch.float64):
    """y = 1.5 + 2 x0 - x1 x2 + 0.5 x0^2 x1 + 0.3 x2^3 on 400 uniform points of [-1, 1]^3: inside the p = 4 candidate set."""
    g = torch.Generator().manual_seed(5)
    X = torch.rand(400, 3, generator=g, dtype=torch.float64) * 2.0 - 1.0
    y = 1.5 + 2.0 * X[:, 0] - X[:, 1] * X[:, 2] + 0.5 * X[:, 0] ** 2 * X[:, 1] + 0.3 * X[:, 2] ** 3
    return X.to(dt), y.to(dt)


def noisy_problem(P, N, seed=None, noise=0.3):
    """(X, y) in fp64: a smooth function of uniform points of [-1, 1]^N plus Gaussian noise."""
    rng = np.random.default_rng(P if seed is None else seed)
    X = rng.uniform(-1.0, 1.0, (P, N))
    y = np.sin(X.sum(axis=1)) + X[:, 0] ** 2 - 0.5 * X[:, 0] * X[:, -1] + noise * rng.standard_normal(P)
    return torch.as_tensor(X), torch.as_tensor(y)


def grid_points(bbox, I, dt, device="cpu"):
    """The I^N cell centres of the bounding box (``to_tensor(domain=I)``'s grid), [I^N, N], first feature slowest."""
    g = [torch.linspace(b[0] + (b[1] - b[0]) / (2 * I), b[1] - (b[1] - b[0]) / (2 * I), I, dtype=dt, device=device) for b in bbox]
    return torch.stack(torch.meshgrid(*g, indexing="ij"), dim=-1).reshape(-1, len(bbox))


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float(torch.norm(a - b) / torch.norm(b))

"""The cases, truths and error bounds the host and the GPU tests of the differentiable ``tn.tt_multiply`` share.

The loss of every case is ``(tt_multiply(ttm, x) * w).sum()`` with a fixed random ``w``: its gradients are multilinear forms in the
remaining operands, so "the same form on absolute values" is autograd of the same chain over ``|x|``, ``|G_k|`` and ``|w|``.

The bounds are derived as in matrix_cases (u = 2^-24 in fp32, 2^-53 in fp64; the factor 2 covers gamma_n <= 2 n u / 1.9):
    one step   |dX - dX64| <= 2 (O S + 1) u (|dY| . |G|)           a dot product of O S terms and the cast
               |dG - dG64| <= 2 (D + 1) u (|X|^T . |dY|)           a dot product of D terms, in any order (so also by slabs)
    the chain  core k: the kept X_k went through the steps before k (sum_{j<k} I_j r_j + k), dY_k through the steps after it
               backwards (sum_{j>k} O_j r_{j+1} + (d - 1 - k)), and the product over D_k adds D_k + 1:
               n = sum_j (I_j r_j + O_j r_{j+1}) + max_k D_k + d + 1 covers every core;
               x: d backward steps of O_j r_{j+1} terms and a cast each: n = sum_j O_j r_{j+1} + d.
"""
import numpy as np
import torch

import matrix_cases as mc

# name -> (case of matrix_cases.RANDOM_CASES, batch or None for the case's own).  "b300": D_k = 4500, 3000, 3600 rows, so on the device
# every ttr_ttm_grad_core of the chain cuts D into 18, 12 and 15 slabs and sums them
GRAD_CASES = {"ref": ("ref", None), "three": ("three", None), "single": ("single", None), "b1": ("three", 1), "b300": ("three", 300)}

_CACHE = {}


def operands(name, dtype):
    """(tt cores, x [b, rows], w [b, cols]) of a GRAD_CASES entry on the CPU, drawn in fp64 and cast."""
    base, b = GRAD_CASES[name]
    tt, _, x = mc.random_cores(base, dtype)
    if b is not None and b <= x.shape[0]:
        x = x[:b].contiguous()
    elif b is not None:
        g = torch.Generator().manual_seed(12)
        x = torch.randn((b, x.shape[1]), dtype=torch.float64, generator=g).to(dtype)
    cols = int(np.prod(mc.RANDOM_CASES[base][1]))
    g = torch.Generator().manual_seed(11)
    w = torch.randn((x.shape[0], cols), dtype=torch.float64, generator=g).to(dtype)
    return tt, x, w


def einsum_chain(cores, x2d):
    """x2d [b, rows] times the TT-matrix, as a chain of einsum calls torch autograd differentiates (independent of the package)."""
    b = x2d.shape[0]
    X = x2d.t().contiguous()
    for G in cores:
        X = torch.einsum("idr,rios->dos", X.reshape(G.shape[1], -1, G.shape[0]), G)
    return X.reshape(b, -1)


def autograd_grads(cores, x, w):
    """(y, [dG_k], dx) of (einsum_chain(cores, x) * w).sum() by torch autograd, in the operands' dtype on their device."""
    cores = [c.detach().clone().requires_grad_(True) for c in cores]
    x = x.detach().clone().requires_grad_(True)
    y = einsum_chain(cores, x)
    (y * w).sum().backward()
    return y.detach(), [c.grad for c in cores], x.grad


def step_rows(cores, b):
    """D_k of every step: b prod_{j > k} I_j prod_{j < k} O_j."""
    I, O = [int(c.shape[1]) for c in cores], [int(c.shape[2]) for c in cores]
    return [b * int(np.prod(I[k + 1:])) * int(np.prod(O[:k])) for k in range(len(cores))]


def truth_and_bounds(name, dtype):
    """(y64, [dG64_k], dx64, [bound of dG_k], bound of dx) in fp64 on the CPU from the operands as rounded to ``dtype``.
    Computed once per (case, dtype) and shared: do not modify."""
    key = (name, dtype)
    if key not in _CACHE:
        tt, x, w = operands(name, dtype)
        tt64, x64, w64 = [c.double() for c in tt], x.double(), w.double()
        y64, dG64, dx64 = autograd_grads(tt64, x64, w64)
        _, magG, magx = autograd_grads([c.abs() for c in tt64], x64.abs(), w64.abs())
        d, u = len(tt), mc.unit(dtype)
        fwd = sum(int(c.shape[1]) * int(c.shape[0]) for c in tt)
        bwd = sum(int(c.shape[2]) * int(c.shape[3]) for c in tt)
        n_core = fwd + bwd + max(step_rows(tt, x.shape[0])) + d + 1
        n_x = bwd + d
        _CACHE[key] = (y64, dG64, dx64, [2 * n_core * u * m for m in magG], 2 * n_x * u * magx)
    return _CACHE[key]


# ------------------------------------------------------------------ one step
def grad_operands(shape, dtype, seed=1):
    """(X [I, D, R], G [R, I, O, S], dY [D, O, S]) on the CPU; X and G are matrix_cases.ttm_operands' for the shape."""
    I, D, R, O, S = shape
    X, G = mc.ttm_operands(shape, dtype, seed)
    g = torch.Generator().manual_seed(seed + 100)
    dY = torch.randn((D, O, S), dtype=torch.float64, generator=g).to(dtype)
    return X, G, dY


def grad_input_truth_and_bound(dY, G, dtype):
    dY, G = dY.detach().double().cpu(), G.detach().double().cpu()
    dX = torch.einsum("dos,rios->idr", dY, G)
    mag = torch.einsum("dos,rios->idr", dY.abs(), G.abs())
    return dX, 2 * (G.shape[2] * G.shape[3] + 1) * mc.unit(dtype) * mag


def grad_core_truth_and_bound(X, dY, dtype):
    X, dY = X.detach().double().cpu(), dY.detach().double().cpu()
    dG = torch.einsum("idr,dos->rios", X, dY)
    mag = torch.einsum("idr,dos->rios", X.abs(), dY.abs())
    return dG, 2 * (X.shape[1] + 1) * mc.unit(dtype) * mag


def small_integers(shape, mul, mod, dtype):
    """An asymmetric tensor of small integers in [-(mod // 2), mod // 2]: products and short sums of them are exact in fp32."""
    n = int(np.prod(shape))
    return ((torch.arange(n) * mul) % mod - mod // 2).to(dtype).reshape(shape)

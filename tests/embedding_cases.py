"""Truths, error bounds and shapes the host and the GPU tests of ``tn.tt_embedding`` / ``tn.tt_embedding_bag`` and of their
kernels (``ttr_ttm_lookup_grad_core``, ``ttr_ttm_lookup_grad_input``, ``ttr_segment_sum``) share.

Every truth is fp64 on the CPU and independent of the package: the einsum of a kernel's contract, or torch autograd through the
dense matrix of the cores (a plain contraction, a gather and a python loop over the bags).  The bounds are derived, not measured
(u = 2^-24 in fp32, 2^-53 in fp64; |.| elementwise; a sum of n products in floating point, in ANY order, is off by at most
gamma_n <= 2 n u / 1.9 times the sum of the magnitudes, and the relative errors of chained steps multiply, (1 + gamma_a)
(1 + gamma_b) <= 1 + gamma_{a + b}; ``matrix_cases`` and ``lookup_cases`` reason the same way):

    grad_core, slice i   |dG - dG64| <= 2 (cnt_i D + nslab_i + 1) u (|X|^T |dY|)     cnt_i D products, the partials of nslab_i slabs
                                                                                      added, one cast
    grad_input           |dX - dX64| <= 2 (O S + 1) u (|dY| . |G|)                   a dot product of O S terms and the cast
    segment_sum          |out - out64| <= 2 u sum |w| |Y|                             fp64 accumulation (fp32: exact products and
                                                                                      len 2^-53 << 2^-24; fp64: compensated) and
                                                                                      the ONE rounding of the result
    a core gradient      |dG_k - dG_k64| <= 2 c_k u mag_k
with mag_k the same gradient evaluated in fp64 with |cores|, |g| and |w|, and c_k the roundings on the longest path from the
operands to an element of dG_k (k counts the cores from 0):
    the forward dots before k      sum_{1 <= j < k} (r_j + 1)                 Z_{k-1}, the left operand of dG_k
    every step after k             sum_{j > k} (O_j r_{j+1} + 1)              the grad_input launches that bring dY_k
    the slice sum                  cnt D_k + nslab + 1  (k = 0: cnt + 1)      cnt = the largest group of digit k
    the bag                        L + 1                                      L = the longest bag (pooled values; 1 without bags)
    weight and mean                2
The value of a pooled row is bounded the same way: 2 (sum_k r_k + d + L + 1 + 2) u (sum |w| |M|[rows])."""
import numpy as np
import torch

import lookup_cases as lc
import matrix_cases as mc

NAMES = ["ref", "three", "single"]
DTYPES = [torch.float32, torch.float64]

# (name, rows are 2-D, mode, weights): the forms of a bag; 1-D rows come with OFFSETS below
BAG_FORMS = [("2d-sum", True, "sum", False), ("2d-mean", True, "mean", False), ("2d-weights", True, "sum", True),
             ("offsets-sum", False, "sum", False), ("offsets-mean", False, "mean", False), ("offsets-weights", False, "sum", True)]
OFFSETS = [0, 0, 3, 3, 7, 12]   # six bags of the 12 rows of lookup_cases.lookup_rows: the first, the third and the last are empty

# ttr_segment_sum: the lengths of the segments (P = 493) and the widths; 63 / 64 / 65 straddle a wave's quarter of 16 rows and
# the unroll of 4, 300 is one long segment, 15 / 80 are no multiple of a 16-byte pack, 80 > the 64 columns of a scalar block
SEG_LENGTHS = [0, 1, 63, 64, 65, 300, 0]
SEG_WIDTHS = [1, 15, 64, 80]


def dense(cores):
    """The dense [rows, cols] matrix of TT-matrix cores by plain contraction, differentiable in the cores."""
    acc = None
    for G in cores:
        acc = G if acc is None else torch.einsum("aiob,bjpc->aijopc", acc, G).reshape(acc.shape[0], acc.shape[1] * G.shape[1],
                                                                                       acc.shape[2] * G.shape[2], G.shape[3])
    return acc[0, :, :, 0]


def case(name, dt):
    """(cores in ``dt`` on the CPU, input dims, output dims, number of rows, number of columns) of a ``matrix_cases`` matrix."""
    idims, odims = mc.RANDOM_CASES[name][:2]
    tt, _, _ = mc.random_cores(name, dt)
    return tt, idims, odims, int(np.prod(idims)), int(np.prod(odims))


def bag_operands(form, nrows, dt):
    """(rows, offsets or None, weights or None, mode, seg) of a bag form; ``seg``: the python list of the B + 1 bag bounds."""
    _, two_d, mode, weighted = form
    rows = lc.lookup_rows(nrows)
    if two_d:
        offsets, seg = None, [0, 6, 12]
    else:
        rows, offsets, seg = rows.reshape(-1), torch.tensor(OFFSETS), OFFSETS + [12]
    w = torch.randn(tuple(rows.shape), dtype=torch.float64, generator=torch.Generator().manual_seed(21)).to(dt) if weighted else None
    return rows, offsets, w, mode, seg


def cotangent(shape, seed=8):
    return torch.randn(shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def pooled(Y, seg, w, mode):
    """[B, cols] from the rows Y [P, cols] by a python loop over the bags; an empty bag is a row of zeros."""
    if seg is None:
        return Y
    if w is not None:
        Y = Y * w.reshape(-1)[:, None]
    out = []
    for b in range(len(seg) - 1):
        s = Y[seg[b]:seg[b + 1]].sum(dim=0)
        out.append(s / max(seg[b + 1] - seg[b], 1) if mode == "mean" else s)
    return torch.stack(out)


def reference(cores, rows, seg, w, mode, g, magnitudes=False):
    """(out, [d out . g / d core]) in fp64 on the CPU by autograd through the dense matrix; ``magnitudes``: the same with |cores|,
    |w| and |g| -- every product then enters with its magnitude, which is what the bounds are relative to."""
    prep = (lambda t: t.detach().double().cpu().abs()) if magnitudes else (lambda t: t.detach().double().cpu())
    leaves = [prep(c).requires_grad_(True) for c in cores]
    rows = torch.as_tensor(rows).cpu().long()
    Y = dense(leaves)[rows.reshape(-1)]
    out = pooled(Y, seg, None if w is None else prep(w), mode)
    out = out if seg is not None else out.reshape(tuple(rows.shape) + (-1,))
    (out * prep(g)).sum().backward()
    return out.detach(), [c.grad for c in leaves]


def digit_counts(idims, rows):
    """The size of the largest group of every digit of the (wrapped) rows, by numpy's unravel_index."""
    total = int(np.prod(idims))
    digits = np.unravel_index(np.asarray(torch.as_tensor(rows).reshape(-1).cpu().numpy()) % total, idims)
    return [int(np.bincount(dg).max()) for dg in digits]


def value_constant(cores, seg):
    """The number of roundings of a (pooled) value: the chain's sum r_k + d, and L + 1 + 2 for a bag."""
    n = sum(int(c.shape[0]) for c in cores) + len(cores)
    if seg is None:
        return n
    return n + max(seg[b + 1] - seg[b] for b in range(len(seg) - 1)) + 1 + 2


def grad_constants(cores, idims, rows, seg, slab_rows):
    """c_k of every core (the docstring's sum); ``slab_rows(k, P, D)``: the slab length of step k's grad_core (k >= 1)."""
    d, P = len(cores), int(torch.as_tensor(rows).numel())
    cnt = digit_counts(idims, rows)
    L = 1 if seg is None else max(seg[b + 1] - seg[b] for b in range(len(seg) - 1))
    out = []
    for k in range(d):
        c = sum(int(cores[j].shape[0]) + 1 for j in range(1, k))
        c += sum(int(cores[j].shape[2]) * int(cores[j].shape[3]) + 1 for j in range(k + 1, d))
        if k == 0:
            c += cnt[0] + 1
        else:
            D = int(np.prod([int(cores[j].shape[2]) for j in range(k)]))
            c += cnt[k] * D + -(-cnt[k] * D // slab_rows(k, P, D)) + 1
        out.append(c + L + 1 + 2)
    return out


# ------------------------------------------------------------------ the kernels
def wrapped(idx, I):
    idx = idx.cpu().long()
    return torch.where(idx < 0, idx + I, idx)


def grad_operands(shape, dt, seed=5, rows_x=None):
    """X [rows_x or P, D, R], G [R, I, O, S], idx [P] in [-I, I) (``lookup_cases.step_operands``) and dY [P, D, O, S]."""
    P, D, R, I, O, S = shape
    X, G, idx = lc.step_operands(shape, dt, seed=seed, rows_x=rows_x)
    dY = torch.randn((P, D, O, S), dtype=torch.float64, generator=torch.Generator().manual_seed(seed + 100)).to(dt)
    return X, G, idx, dY


def grad_core_truth_and_bound(X, xrow, dY, idx, I, slab_rows, dt):
    """dG64 [R, I, O, S] by the einsum of the contract, and 2 (cnt_i D + nslab_i + 1) u |X|^T |dY| slice by slice; also cnt."""
    X, dY = X.detach().double().cpu(), dY.detach().double().cpu()
    Xg = X if xrow is None else X[xrow.cpu().long()]
    v = wrapped(idx, I)
    R, D = X.shape[2], X.shape[1]
    zeros = lambda: torch.zeros((R, I, dY.shape[2], dY.shape[3]), dtype=torch.float64)
    dG = zeros().index_add_(1, v, torch.einsum("pdr,pdos->rpos", Xg, dY))
    mag = zeros().index_add_(1, v, torch.einsum("pdr,pdos->rpos", Xg.abs(), dY.abs()))
    cnt = torch.bincount(v, minlength=I)
    n = cnt * D + (cnt * D + slab_rows - 1) // slab_rows + 1
    return dG, 2 * n.double()[None, :, None, None] * mc.unit(dt) * mag, cnt


def grad_input_truth_and_bound(dY, G, idx, dt):
    dY, G = dY.detach().double().cpu(), G.detach().double().cpu()
    Gg = G[:, wrapped(idx, G.shape[1])]
    dX = torch.einsum("pdos,rpos->pdr", dY, Gg)
    mag = torch.einsum("pdos,rpos->pdr", dY.abs(), Gg.abs())
    return dX, 2 * (G.shape[2] * G.shape[3] + 1) * mc.unit(dt) * mag


def segment_operands(C, dt, seed=31):
    """Y [493, C], w [493], a random permutation and the bounds of SEG_LENGTHS."""
    g = torch.Generator().manual_seed(seed)
    P = sum(SEG_LENGTHS)
    Y = torch.randn((P, C), dtype=torch.float64, generator=g).to(dt)
    w = torch.randn((P,), dtype=torch.float64, generator=g).to(dt)
    perm = torch.randperm(P, generator=g)
    seg = torch.tensor([0] + list(np.cumsum(SEG_LENGTHS)), dtype=torch.int64)
    return Y, w, perm, seg


def segment_truth_and_bound(Y, seg, w, perm, dt):
    """(out64, bound).  The kernel's fp64 result carries ONE rounding, so a plain fp64 sum of up to 300 terms (off by up to
    len u itself) is no truth for it: the products and the sums run in numpy's extended precision (64-bit mantissa where the
    platform has it) and the result is rounded to fp64 once.  That rounding (u |out|) and the kernel's (u |out|) fill the bound."""
    Yl = Y.detach().double().cpu().numpy().astype(np.longdouble)
    rows = Yl if perm is None else Yl[perm.cpu().numpy()]
    if w is not None:
        wl = w.detach().double().cpu().numpy().astype(np.longdouble)
        rows = rows * (wl if perm is None else wl[perm.cpu().numpy()])[:, None]
    bounds = seg.tolist()
    part = lambda a, b: a[bounds[b]:bounds[b + 1]].sum(axis=0)   # (an empty slice sums to zeros)
    out = np.stack([part(rows, b) for b in range(len(bounds) - 1)]).astype(np.float64)
    mag = np.stack([part(np.abs(rows), b) for b in range(len(bounds) - 1)]).astype(np.float64)
    return torch.from_numpy(out), 2 * mc.unit(dt) * torch.from_numpy(mag)

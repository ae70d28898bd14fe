"""Host (CPU tensor) mirror of the hot path, on batch-normalised ``[B, ...]`` tensors.

This is the "plumbing" path of BASELINE config C0 (``tn.Tensor(torch.randn(16,16,16,16))
.round_tt(rmax=4)`` on CPU PyTorch): same operator sequence as the reference
(torch.linalg.qr / svd / eigh on the CPU), so CPU results agree with the reference to
round-off.  It is selected ONLY for CPU tensors; device tensors never come here
(``_dispatch.ops_for`` raises instead of falling back).
"""

from __future__ import annotations

import math
import time
from typing import List, Optional, Sequence, Tuple

import torch

INT32_MAX = 2**31 - 1
VERBOSE = False   # set by the API layer around a call with verbose=True: the reference's per-stage timing lines (round.py:95-117, 163-185; tensor.py:2032-2035)


def _t(M):
    return M.transpose(-1, -2)


def qr(A3: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """tensor.py:1816 (reduced QR).  A single matrix goes through the 2-D LAPACK path exactly as in
    the reference's non-batch mode, so CPU results match the reference bit for bit."""
    if A3.shape[0] == 1:
        Q, R = torch.linalg.qr(A3[0])
        return Q[None], R[None]
    return torch.linalg.qr(A3)


def _mm(A, B):
    if A.dim() == 3 and A.shape[0] == 1:
        return (A[0] @ B[0])[None]
    return A @ B


def truncated_svd(M3, delta, eps, rmax, left_ortho, algorithm, batch):
    """round.py:52-187 with the batch dim always present ([B, m, n]; B == 1 when not batch)."""
    if not batch:  # same 2-D operator calls as the reference's non-batch mode
        left, M2 = _truncated_svd(M3, delta, eps, rmax, left_ortho, algorithm, False, squeeze=True)
        return left, M2
    return _truncated_svd(M3, delta, eps, rmax, left_ortho, algorithm, True, squeeze=False)


def _truncated_svd(M3, delta, eps, rmax, left_ortho, algorithm, batch, squeeze):
    if squeeze:
        M3 = M3[0]
        lead = ()
    else:
        lead = (M3.shape[0],)
    if delta is None and eps is not None:  # round.py:79-80
        delta = eps * torch.norm(M3).item()
    if delta is None:
        delta = 0
    if rmax is None:
        rmax = INT32_MAX
    m, n = M3.shape[-2], M3.shape[-1]

    start = time.time()
    if algorithm == "svd":  # round.py:94-100
        U, sig = torch.linalg.svd(M3)[:2]
        side = "left"
        if VERBOSE:
            print("Time (SVD):", time.time() - start)
    else:  # round.py:101-135
        if m <= n:
            gram, side = M3 @ _t(M3), "left"
        else:
            gram, side = _t(M3) @ M3, "right"
        if VERBOSE:
            print("Time (gram):", time.time() - start)
        start = time.time()
        w, U = torch.linalg.eigh(gram)
        if VERBOSE:
            print("Time (symmetric EIG):", time.time() - start)
        w = torch.where(w < 0, torch.zeros_like(w) + 1e-8, w)
        sig = torch.sqrt(w)
        sig, idx = torch.sort(sig, dim=-1, descending=True)
        U = torch.gather(U, -1, idx[..., None, :].expand(U.shape))

    if sig.max() < 1e-13:  # round.py:137-145 (kept on M's device/dtype)
        return M3.new_zeros((1,) * squeeze + lead + (m, 1)), M3.new_zeros((1,) * squeeze + lead + (1, n))

    S = sig**2
    k = S.shape[-1]
    if batch:  # round.py:149-150
        rank = max(1, int(min(rmax, k)))
    else:  # round.py:152-158
        tail = torch.cumsum(torch.flip(S, [0]), dim=0) <= delta**2
        where = torch.where(tail)[0]
        if len(where) == 0:
            rank = max(1, int(min(rmax, k)))
        else:
            rank = max(1, int(min(rmax, k - 1 - int(where[-1]))))

    left = U[..., :rank]
    sr = sig[..., :rank].to(M3.dtype)
    start = time.time()
    if side == "left":  # round.py:164-172
        if left_ortho:
            M2 = _t(left) @ M3
        else:
            M2 = (1.0 / sr)[..., None] * _t(left) @ M3
            left = left * sr[..., None, :]
    else:  # round.py:173-182
        if left_ortho:
            newleft = M3 @ (left * (1.0 / sr)[..., None, :])
            M2 = _t(left * sr[..., None, :])
            left = newleft
        else:
            newleft = M3 @ left
            M2 = _t(left)
            left = newleft
    if VERBOSE:
        print("Time (product):", time.time() - start)
    if squeeze:
        return left[None], M2[None]
    return left, M2


def mode_mul(core4: torch.Tensor, M3: torch.Tensor, trans: bool = False) -> torch.Tensor:
    """[B, r0, S, r1] x_2 [B, a, S] -> [B, r0, a, r1] (the einsum of tensor.py:1790-1798, 1999-2002); ``trans``: the matrix is
    given as [B, S, a] (a view: it is not copied)."""
    if trans:
        M3 = M3.transpose(1, 2)
    if core4.shape[0] == 1:
        return torch.einsum("ijk,aj->iak", core4[0], M3[0])[None]
    return torch.einsum("bijk,baj->biak", core4, M3)


def merge_swap(c1: torch.Tensor, c2: torch.Tensor) -> torch.Tensor:
    """Two neighbouring cores [B, R1, I1, R2], [B, R2, I2, R3] contracted over the bond with their modes exchanged:
    ``einsum("iaj,jbk->ibak")`` flattened to [B, R1*I2, I1*R3] (tools.py:680-681)."""
    sc = torch.einsum("ziaj,zjbk->zibak", c1, c2)
    return sc.reshape(sc.shape[0], sc.shape[1] * sc.shape[2], sc.shape[3] * sc.shape[4])


def diag_sum(core5: torch.Tensor) -> torch.Tensor:
    """[B, r0, a, a, r1] -> [B, r0, r1]: sum of the slices on the diagonal of the two mode axes (matrix.py:160-175)."""
    return torch.einsum("ziaaj->zij", core5)


def factor_orthogonalize(c: List[torch.Tensor], Us, mu: int) -> None:
    """tensor.py:1771-1798: QR of the Tucker factor [B, I, S], R pushed into the core."""
    if Us is None or Us[mu] is None:
        return
    Q, R = qr(Us[mu])
    Us[mu] = Q
    c[mu] = mode_mul(c[mu], R)


def left_orthogonalize(c: List[torch.Tensor], mu: int, Us=None) -> torch.Tensor:
    """tensor.py:1800-1833 on [B, r0, I, r1] cores."""
    factor_orthogonalize(c, Us, mu)
    Bt, r0, I, r1 = c[mu].shape
    Q, R = qr(c[mu].reshape(Bt, r0 * I, r1))
    k = Q.shape[2]
    c[mu] = Q.reshape(Bt, r0, I, k)
    nxt = c[mu + 1]
    c[mu + 1] = _mm(R, nxt.reshape(Bt, nxt.shape[1], -1)).reshape(Bt, k, nxt.shape[2], nxt.shape[3])
    return R


def right_orthogonalize(c: List[torch.Tensor], mu: int, Us=None) -> torch.Tensor:
    """tensor.py:1835-1879."""
    factor_orthogonalize(c, Us, mu)
    Bt, r0, I, r1 = c[mu].shape
    Q, Lt = qr(_t(c[mu].reshape(Bt, r0, I * r1)))
    Q, L = _t(Q), _t(Lt)
    k = Q.shape[1]
    c[mu] = Q.reshape(Bt, k, I, r1)
    prev = c[mu - 1]
    c[mu - 1] = _mm(prev.reshape(Bt, prev.shape[1] * prev.shape[2], r0), L).reshape(Bt, prev.shape[1], prev.shape[2], k)
    return L


def round_tt(cores4: Sequence[torch.Tensor], eps, rmax, algorithm, batch, Us=None) -> List[torch.Tensor]:
    """tensor.py:2008-2083 (``Us``: Tucker factors, orthogonalised in place by the L2R sweep)."""
    c = list(cores4)
    N = len(c)
    start = time.time()
    for mu in range(N - 1):
        left_orthogonalize(c, mu, Us)
    if VERBOSE:
        print("Orthogonalization time:", time.time() - start)
    if batch:
        delta = None
    else:
        delta = (eps / max(1.0, math.sqrt(N - 1))) * float(torch.norm(c[-1]).double().item())
    for mu in range(N - 1, 0, -1):
        Bt, R, I, rn = c[mu].shape
        left, right = truncated_svd(c[mu].reshape(Bt, R, I * rn), delta, None, rmax[mu - 1], False, algorithm, batch)
        left, right = left.to(c[mu].dtype), right.to(c[mu].dtype)
        r = right.shape[1]
        c[mu] = right.reshape(Bt, r, I, rn)
        prev = c[mu - 1]
        c[mu - 1] = _mm(prev.reshape(Bt, prev.shape[1] * prev.shape[2], R), left).reshape(Bt, prev.shape[1], prev.shape[2], r)
    return c


def round_tucker(cores4: Sequence[torch.Tensor], Us, eps, rmax, ndims, algorithm, batch):
    """tensor.py:1911-2006 on [B, r0, S, r1] cores and [B, I, S] factors; returns (cores, Us)."""
    c = list(cores4)
    N = len(c)
    Us = [None] * N if Us is None else list(Us)
    for i in range(N - 1):  # orthogonalize(-1), tensor.py:1944
        left_orthogonalize(c, i, Us)
    for mu in range(N - 1, -1, -1):
        Bt, r0, S, r1 = c[mu].shape
        if Us[mu] is None:  # tensor.py:1946-1958
            Us[mu] = torch.eye(S, dtype=c[mu].dtype, device=c[mu].device).repeat(Bt, 1, 1)
        Q, R = qr(c[mu].permute(0, 1, 3, 2).reshape(Bt, r0 * r1, S))  # tensor.py:1960-1984
        c[mu] = Q.reshape(Bt, r0, r1, Q.shape[2]).permute(0, 1, 3, 2)
        Us[mu] = _mm(Us[mu], _t(R))  # tensor.py:1986
        left, right = truncated_svd(Us[mu], None, eps / math.sqrt(ndims), rmax[mu], True, algorithm, batch)
        Us[mu] = left.to(c[mu].dtype)
        c[mu] = mode_mul(c[mu], right.to(c[mu].dtype))  # tensor.py:1999-2002
        if mu > 0:
            right_orthogonalize(c, mu, Us)
    return c, Us


def absorb_factors(cores4: Sequence[torch.Tensor], Us) -> List[torch.Tensor]:
    """Contract every Tucker factor into its core (what tensor.py:1639-1687 does per mode)."""
    return [c if U is None else mode_mul(c, U) for c, U in zip(cores4, Us)]


def dense_tucker_tt(X: torch.Tensor, ranks_tucker, ranks_tt, algorithm, batch):
    """tensor.py:401-408: full-rank TT, ``round_tucker(rmax=ranks_tucker)``, ``round_tt(rmax=ranks_tt)``."""
    c = full_rank_tt(X)
    N = len(c)
    c, Us = round_tucker(c, None, 1e-14, ranks_tucker, N, algorithm, batch)
    if ranks_tt is not None:
        c = round_tt(c, 1e-14, ranks_tt, algorithm, batch, Us)
    return c, Us


def full_rank_tt(X: torch.Tensor) -> List[torch.Tensor]:
    """tensor.py:10-104 on a batch-normalised dense tensor [B, I_1..I_N] (views/eye only)."""
    Bt = X.shape[0]
    shape = list(X.shape[1:])
    N = len(shape)

    def eye(n):
        return torch.eye(n, dtype=X.dtype, device=X.device).repeat(Bt, 1, 1)

    resh = X.reshape(Bt, shape[0], -1)
    out = []
    for n in range(1, N):
        rows, cols = resh.shape[1], resh.shape[2]
        if rows < cols:
            out.append(eye(rows).reshape(Bt, rows // shape[n - 1], shape[n - 1], rows))
            resh = resh.reshape(Bt, rows * shape[n], cols // shape[n])
        else:
            out.append(resh.reshape(Bt, rows // shape[n - 1], shape[n - 1], cols))
            resh = eye(cols).reshape(Bt, cols * shape[n], cols // shape[n])
    rows = resh.shape[1]
    out.append(resh.reshape(Bt, rows // shape[N - 1], shape[N - 1], 1))
    return out


def dense_tt_svd(X: torch.Tensor, eps, rmax, algorithm, batch) -> List[torch.Tensor]:
    """tensor.py:401-408 exactly as the reference does it: full-rank TT, then round_tt."""
    return round_tt(full_rank_tt(X), eps, rmax, algorithm, batch)


# ---------------------------------------------------------------------------------------------- consumers
def decompress(c: Sequence[torch.Tensor]) -> torch.Tensor:
    """tensor.py:1639-1687 for TT cores [B, r0, I, r1] -> [B, I_1, ..., I_N]."""
    Bt = c[0].shape[0]
    acc = c[0].reshape(Bt, -1, c[0].shape[-1])
    for core in c[1:]:
        acc = torch.bmm(acc, core.reshape(Bt, core.shape[1], -1)).reshape(Bt, -1, core.shape[-1])
    # ranks_tt[0] and ranks_tt[-1] may exceed 1: the reference sums the boundary indices away
    r0 = c[0].shape[1]
    acc = acc.reshape(Bt, r0, -1, c[-1].shape[-1]).sum(dim=(1, 3))
    return acc.reshape([Bt] + [core.shape[2] for core in c])


def dot(c1: Sequence[torch.Tensor], c2: Sequence[torch.Tensor]) -> torch.Tensor:
    """metrics.py:28-116 (k = N, TT cores only) on cores [1, r, I, r']."""
    a0, b0 = c1[0][0], c2[0][0]
    L = torch.ones([b0.shape[0], a0.shape[0]], device=a0.device, dtype=a0.dtype)
    for a, b in zip(c1, c2):
        a, b = a[0], b[0]
        U = torch.einsum("sr,rai->sai", L, a)
        L = b.reshape(-1, b.shape[-1]).t() @ U.reshape(-1, U.shape[-1])
    return torch.sum(L)


def dense_dot(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return a.flatten().dot(b.flatten())


# ---------------------------------------------------------------------------------------------- moments (metrics.py:345-455)
def core_matvec(x: torch.Tensor, G: torch.Tensor) -> torch.Tensor:
    """metrics.py:434-445: TT-matrix core G [A, K, S, C] times TT-vector core x [P, K, Q] -> [P A, S, Q C],
    out[p A + a, s, q C + c] = sum_k x[p, k, q] G[a, k, s, c]."""
    P, K, Q = x.shape
    A, _, S, C = G.shape
    return torch.einsum("pkq,aksc->pasqc", x, G).reshape(P * A, S, Q * C)


def hsum_step(W: torch.Tensor, cores: Sequence[torch.Tensor]) -> torch.Tensor:
    """metrics.py:407-425, one mode: W [r_1, .., r_K], cores A_m [r_m, I, r'_m] -> W' [r'_1, .., r'_K],
    W'[a'] = sum_i sum_a W[a] prod_m A_m[a_m, i, a'_m]."""
    K = len(cores)
    I = cores[0].shape[1]
    T = W[None].expand((I,) + tuple(W.shape))
    for m, A in enumerate(cores):  # mode product m on the view [I, left, r_m, right]; the mode index i is a batch index
        left = math.prod(T.shape[1:1 + m])
        T3 = T.reshape(I, left, A.shape[0], -1)
        T = torch.einsum("ilar,aib->ilbr", T3, A).reshape(tuple(T.shape[:1 + m]) + (A.shape[2],) + tuple(T.shape[2 + m:]))
    return T.sum(dim=0)


def diag_cores(cs: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    """metrics.py:358-382 (``diag_core`` / ``get_tensor`` before its rounding): the cores c_m [Rl_m, I, Rr_m] of ONE mode of M
    trains -> the M cores [1, I or 1, Rl_m Rr_m, I or 1] of the train over the rank pairs whose bond is the mode index,
    D_m[i, (a, b), j] = delta_ij c_m[a, i, b] (summed over i for m = 0 and over j for m = M - 1).  Index plumbing: I Rl Rr
    values are scattered into zeros -- torch does it on whichever device the cores live."""
    M = len(cs)
    out = []
    for m, c in enumerate(cs):
        Rl, I, Rr = c.shape
        F = c.permute(1, 0, 2).reshape(I, Rl * Rr)
        if M == 1:
            D = F.sum(dim=0).reshape(1, Rl * Rr, 1)
        elif m == 0:
            D = F.t()[None]
        elif m == M - 1:
            D = F[:, :, None]
        else:
            D = c.new_zeros((I, Rl * Rr, I))
            idx = torch.arange(I, device=c.device)
            D[idx, :, idx] = F
        out.append(D.contiguous()[None])
    return out


def sum_all(x: torch.Tensor) -> torch.Tensor:
    return x.sum()


def dense_norm(a: torch.Tensor) -> torch.Tensor:
    return torch.norm(a)


def dense_dist(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return torch.dist(a, b)


# ---------------------------------------------------------------------------------------------- core gradients from samples
GRAD_TASK_SAMPLES = 4096  # samples per ttr_gather_grad task: longer slices are split, so skewed data does not sit on one workgroup


class GradPlan:
    """The tasks of one mode for ``ttr_gather_grad``: slice i with n samples becomes ceil(n / task_samples) tasks of nearly equal
    length (AlsPlan's splitting rule), a slice without samples gets none.  Built on the host from the per-slice counts and
    uploaded once."""

    def __init__(self, counts: Sequence[int], device, task_samples: Optional[int] = None):
        ts = int(GRAD_TASK_SAMPLES if task_samples is None else task_samples)
        if ts < 1:
            raise ValueError("GradPlan: task_samples must be at least 1")
        tb, te, toff, pos = [], [], [0], 0
        for n in counts:
            n = int(n)
            nt = -(-n // ts)
            for k in range(nt):
                tb.append(pos + (n * k) // nt)
                te.append(pos + (n * (k + 1)) // nt)
            pos += n
            toff.append(len(tb))
        self.ntasks, self.nslices, self.nsamples = len(tb), len(toff) - 1, pos
        self.tb = torch.tensor(tb, dtype=torch.int64, device=device)
        self.te = torch.tensor(te, dtype=torch.int64, device=device)
        self.toff = torch.tensor(toff, dtype=torch.int64, device=device)


def gather_grad(L: torch.Tensor, R: torch.Tensor, perm: torch.Tensor, plan: GradPlan) -> torch.Tensor:
    """Mirror of ttr_gather_grad: dG [r0, I, r1], dG[:, i, :] = sum of L[p]^T R[p] over the samples of slice i, i.e. over the runs
    perm[tb[t]:te[t]] of the slice's tasks (``index_add_`` of the outer products; any float dtype)."""
    r0, r1, I = L.shape[1], R.shape[1], plan.nslices
    owner = torch.repeat_interleave(torch.arange(I, device=L.device), plan.toff[1:] - plan.toff[:-1])  # slice of each task
    lens = plan.te - plan.tb
    pos = torch.repeat_interleave(plan.tb, lens) + (torch.arange(int(lens.sum()), device=L.device)
                                                   - torch.repeat_interleave(torch.cumsum(lens, 0) - lens, lens))
    q = perm[pos]
    dG = torch.zeros((I, r0, r1), dtype=L.dtype, device=L.device)
    dG.index_add_(0, torch.repeat_interleave(owner, lens), L[q, :, None] * R[q, None, :])
    return dG.permute(1, 0, 2).contiguous()


# ---------------------------------------------------------------------------------------------- derivatives (derivatives.py:72-302)
def _diff_pass(X: torch.Tensor, periodic: bool, inv_step: float) -> torch.Tensor:
    """One pass of derivatives.py:96-129 on X [R, I, C]: interior rows x[i+1] - x[i-1], rows 0 and I-1 twice the one-sided
    difference (the reference's linearly extrapolated edge), or roll(-1) - roll(+1); times inv_step."""
    I = X.shape[1]
    if periodic:
        return (torch.roll(X, -1, 1) - torch.roll(X, 1, 1)) * inv_step
    Y = torch.zeros_like(X)
    if I == 1:
        return Y
    Y[:, 1:-1] = X[:, 2:] - X[:, :-2]
    Y[:, 0] = 2 * (X[:, 1] - X[:, 0])
    Y[:, -1] = 2 * (X[:, -1] - X[:, -2])
    return Y * inv_step


def mode_diff(X: torch.Tensor, order: int, periodic: bool, inv_step: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Mirror of ttr_mode_diff: ``order`` passes along the middle axis of X [R, I, C]; ``out`` (a [R, I, C] view) receives the result."""
    if order < 1:
        raise ValueError("mode_diff: order {} < 1".format(order))
    Y = X.double()   # as the kernel: the passes run in fp64 for both dtypes, one rounding at the end
    for _ in range(int(order)):
        Y = _diff_pass(Y, periodic, inv_step)
    Y = Y.to(X.dtype)
    if out is None:
        return Y
    out.copy_(Y)
    return out


def laplace_core(X: torch.Tensor, pos: int, periodic: bool, inv_step: float) -> torch.Tensor:
    """Mirror of ttr_laplace_core: pos 0 [X D] ([R, I, 2C]), 1 [[X, D], [0, X]] ([2R, I, 2C]), 2 [D ; X] ([2R, I, C]),
    D = (inv_step S)^2 X."""
    R, I, C = X.shape
    if pos == 2:
        out = X.new_empty((2 * R, I, C))
        mode_diff(X, 2, periodic, inv_step, out=out[:R])
        out[R:] = X
        return out
    out = X.new_zeros(((2 if pos == 1 else 1) * R, I, 2 * C))
    out[:R, :, :C] = X
    mode_diff(X, 2, periodic, inv_step, out=out[:R, :, C:])
    if pos == 1:
        out[R:, :, C:] = X
    return out


# ---------------------------------------------------------------------------------------------- array tools (ops.py:6-30, tools.py:266-325)
def mode_scan(X: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Mirror of ttr_mode_scan: the running sum along the middle axis of X [R, I, C], accumulated in fp64 and rounded once;
    ``out`` (a [R, I, C] view) receives the result."""
    Y = torch.cumsum(X.double(), dim=1).to(X.dtype)
    if out is None:
        return Y
    out.copy_(Y)
    return out


def mode_reduce(X: torch.Tensor, w: Optional[torch.Tensor] = None, scale: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Mirror of ttr_mode_reduce: Y[r, c] = scale * sum_i w[i] X[r, i, c] for X [R, I, C] (``w`` None: all ones), accumulated in
    fp64 and rounded once; ``out`` (a [R, C] view) receives the result."""
    Xd = X.double()
    Y = Xd.sum(dim=1) if w is None else torch.einsum("i,ric->rc", w.double(), Xd)
    Y = (Y * float(scale)).to(X.dtype)
    if out is None:
        return Y
    out.copy_(Y)
    return out


# ---------------------------------------------------------------------------------------------- ANOVA / Sobol (anova.py:99-148)
def mode_sandwich(Z: torch.Tensor, A: torch.Tensor, w: Optional[torch.Tensor] = None, mu: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Mirror of ttr_mode_sandwich: Z [S, R, R], A [R, I, C], w [I] or None (ones), mu [R, C] or None (zeros) -> Q [S, C, C],
    Q[s] = sum_i w[i] (A_i - mu)^T Z[s] (A_i - mu): two einsums in the input dtype."""
    Ac = A if mu is None else A - mu[:, None, :]
    Y = torch.einsum("sab,bic->saic", Z, Ac)
    if w is not None:
        Y = Y * w[None, None, :, None]
    return torch.einsum("aic,said->scd", Ac, Y)


# ---------------------------------------------------------------------------------------------- polynomial chaos (interpolation.py:347-630)
PCE_CHUNK = 1 << 14  # points per pass of the mirrors below: the largest intermediate is PCE_CHUNK x max(C, N S) in fp64


def _pce_check(Z: torch.Tensor, Psi: torch.Tensor, coords: torch.Tensor):
    if Z.dim() != 2 or Psi.dim() != 3 or Psi.shape[0] != Z.shape[1] or Psi.shape[1] != Psi.shape[2] or Psi.dtype != Z.dtype:
        raise ValueError("pce: expected Z [P, N] and Psi [N, S, S] of one dtype")
    if coords.dim() != 2 or coords.shape[1] != Z.shape[1] or coords.dtype.is_floating_point:
        raise ValueError("pce: coords must be an integer [C, N] matrix")
    S = int(Psi.shape[1])
    if coords.numel() and (int(coords.min()) < 0 or int(coords.max()) >= S):
        raise ValueError("pce: coordinates outside [0, {})".format(S))


def _pce_basis(Z: torch.Tensor, Psi: torch.Tensor) -> torch.Tensor:
    """B[p, n, s] = sum_k Z[p, n]^k Psi[n, k, s] in fp64, by Horner from k = S - 1 down (the order of the kernels)."""
    Zd, Pd = Z.double()[:, :, None], Psi.double()
    S = Pd.shape[1]
    acc = Pd[None, :, S - 1, :].expand(Zd.shape[0], -1, -1)
    for k in range(S - 2, -1, -1):
        acc = acc * Zd + Pd[None, :, k, :]
    return acc


def pce_moments(Z: torch.Tensor, S: int) -> torch.Tensor:
    """H[n] = V_n^T V_n / P with V_n[p, k] = Z[p, n]^k: the empirical moment matrices [N, S, S] of the columns of Z, in fp64."""
    P, N = Z.shape
    H = torch.zeros(N, S, S, dtype=torch.float64, device=Z.device)
    ks = torch.arange(S, device=Z.device)
    for lo in range(0, P, PCE_CHUNK):
        V = Z[lo : lo + PCE_CHUNK].double().t()[:, :, None] ** ks   # [N, chunk, S]
        H += _t(V) @ V
    return H / P


def _pce_products(Z: torch.Tensor, Psi: torch.Tensor, coords: torch.Tensor):
    """(first row, fp64 products [rows, C]) of one chunk of PCE_CHUNK points after the other: no P x C x N intermediate."""
    _pce_check(Z, Psi, coords)
    coords = coords.long()
    for lo in range(0, Z.shape[0], PCE_CHUNK):
        B = _pce_basis(Z[lo : lo + PCE_CHUNK], Psi)
        prod = B[:, 0, :][:, coords[:, 0]]
        for n in range(1, Z.shape[1]):
            prod = prod * B[:, n, :][:, coords[:, n]]
        yield lo, prod


def pce_design(Z: torch.Tensor, Psi: torch.Tensor, coords: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Mirror of ttr_pce_design: M[p, c] = prod_n B(p, n, coords[c, n]) for Z [P, N], Psi [N, S, S], coords [C, N], computed in
    fp64 (n increasing) and rounded once.  ValueError for a coordinate outside [0, S).  ``out`` (a [P, C] view) receives the
    result."""
    M = out if out is not None else torch.empty((Z.shape[0], coords.shape[0]), dtype=Z.dtype, device=Z.device)
    for lo, prod in _pce_products(Z, Psi, coords):
        M[lo : lo + PCE_CHUNK] = prod.to(Z.dtype)
    return M


def pce_predict(Z: torch.Tensor, Psi: torch.Tensor, coords: torch.Tensor, coef: torch.Tensor, check: bool = True) -> torch.Tensor:
    """Mirror of ttr_pce_predict: y[p] = sum_c coef[c] prod_n B(p, n, coords[c, n]), in fp64 and rounded once."""
    y = torch.empty(Z.shape[0], dtype=Z.dtype, device=Z.device)
    cd = coef.double()
    for lo, prod in _pce_products(Z, Psi, coords):
        y[lo : lo + PCE_CHUNK] = (prod @ cd).to(Z.dtype)
    return y


def pce_gram(M: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """[M | y]^T M as one [C + 1, C] matrix in M's dtype: rows 0 .. C - 1 are the Gram matrix M^T M, row C is M^T y -- all that
    LARS needs of the P rows, in one tensor (one copy to the host)."""
    return torch.cat([M.t() @ M, (y @ M)[None]], dim=0)


# ---------------------------------------------------------------------------------------------- convolution (tools.py:579-647)
def core_convolve(a: torch.Tensor, c: torch.Tensor, lo: int, K: int) -> torch.Tensor:
    """Mirror of ttr_core_convolve: a [R1, I, R2], c [S1, J, S2] -> [R1 S1, K, R2 S2],
    out[r1 S1 + s1, k, r2 S2 + s2] = sum_i a[r1, i, r2] c[s1, k + lo - i, s2] for the window 0 <= lo, lo + K <= I + J - 1 of the
    full result.  One shifted multiply-add per index of the SHORTER mode, in increasing order, accumulated in the input dtype."""
    if a.dim() != 3 or c.dim() != 3 or a.dtype != c.dtype or a.device != c.device:
        raise ValueError("core_convolve: expected two 3-d cores of one dtype on one device")
    R1, I, R2 = a.shape
    S1, J, S2 = c.shape
    lo, K = int(lo), int(K)
    if min(R1, I, R2, S1, J, S2, K) < 1 or lo < 0 or lo + K > I + J - 1:
        raise ValueError("core_convolve: bad sizes or window (lo = {}, K = {}) for modes {} and {}".format(lo, K, I, J))
    out = a.new_zeros((R1, S1, K, R2, S2))
    swap = J < I   # the roles are symmetric: sum_j c[j] a[k + lo - j]
    short, long_ = (c, a) if swap else (a, c)
    Q = long_.shape[1]
    for p in range(short.shape[1]):
        k0, k1 = max(0, p - lo), min(K, Q + p - lo)   # the k with 0 <= k + lo - p < Q
        if k1 <= k0:
            continue
        x, y = short[:, p, :], long_[:, k0 + lo - p:k1 + lo - p, :]
        if swap:
            out[:, :, k0:k1] += x[None, :, None, None, :] * y[:, None, :, :, None]
        else:
            out[:, :, k0:k1] += x[:, None, None, :, None] * y[None, :, :, None, :]
    return out.reshape(R1 * S1, K, R2 * S2)


def core_compose(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """Mirror of ttr_core_compose: A [R1, P, J, R2], B [S1, J, Q, S2] -> [R1 S1, P, Q, R2 S2],
    out[r S1 + a, p, q, s S2 + b] = sum_j A[r, p, j, s] B[a, j, q, b].  One einsum in the input dtype: differentiable."""
    if A.dim() != 4 or B.dim() != 4 or A.dtype != B.dtype or A.device != B.device:
        raise ValueError("core_compose: expected two 4-d cores of one dtype on one device")
    if A.shape[2] != B.shape[1]:
        raise ValueError("core_compose: A [R1, P, J, R2] and B [S1, J, Q, S2] need the same J, got {} and {}".format(A.shape[2], B.shape[1]))
    R1, P, _, R2 = A.shape
    S1, _, Q, S2 = B.shape
    return torch.einsum("rpjs,ajqb->rapqsb", A, B).reshape(R1 * S1, P, Q, R2 * S2)


# ---------------------------------------------------------------------------------------------- CP-ALS
def cp_als(X: torch.Tensor, R: int, max_iter: int, tol: float, verbose: bool = False, batch: bool = False, init=None):
    """tensor.py:210-400, the reference's operator sequence on the CPU.  ``init=None``: HOSVD initialisation
    (tensor.py:228-277); otherwise the given factors (CP on a Tucker core starts from ``randn``, tensor.py:282-300).
    ``batch``: X is [B, I_1..I_N], factors are [B, I_n, R], ONE convergence decision on the batch-mean error."""
    if batch:
        return _cp_als_batch(X, R, max_iter, tol, verbose, init)
    N = X.dim()

    def unf(n):
        return X.permute([n] + list(range(n)) + list(range(n + 1, N))).reshape(X.shape[n], -1)

    if init is not None:
        A = list(init)
    else:
        A = []
        for n in range(N):  # tensor.py:228-277
            g = unf(n)
            g = g @ _t(g)
            w, V = torch.linalg.eigh(g)
            reverse = torch.arange(len(w) - 1, -1, -1)
            idx = torch.argsort(w)[reverse[:R]]
            c = V[:, idx]
            if c.shape[1] < R:
                c = torch.cat((c, torch.randn(c.shape[0], R - c.shape[1], dtype=c.dtype, device=c.device)), dim=1)
            A.append(c)
    xnorm = torch.norm(X)
    grams = [None] + [_t(A[n]) @ A[n] for n in range(1, N)]
    errors = []
    for it in range(max_iter):
        for n in range(N):
            khatri = torch.ones(1, R, dtype=X.dtype, device=X.device)
            prod = torch.ones(R, R, dtype=X.dtype, device=X.device)
            for m in range(N - 1, -1, -1):
                if m != n:
                    prod *= grams[m]
                    khatri = torch.reshape(torch.einsum("ir,jr->ijr", (A[m], khatri)), [-1, R])
            A[n] = _t(torch.linalg.lstsq(prod, _t(unf(n) @ khatri)).solution)
            grams[n] = _t(A[n]) @ A[n]
        acc = A[0]
        for c in A[1:]:
            acc = torch.einsum("ar,ir->air", acc, c).reshape(-1, R)
        errors.append(float(torch.norm(X - acc.sum(dim=1).reshape(X.shape)) / xnorm))
        if verbose:
            print("iter: {} | eps: {:.8f}".format(it, errors[-1]))
        if len(errors) >= 2 and errors[-2] - errors[-1] < tol:
            break
    return A, errors


def _cp_als_batch(X: torch.Tensor, R: int, max_iter: int, tol: float, verbose: bool, init):
    """The ``batch=True`` branches of tensor.py:214-400: every product is a ``bmm`` over the leading axis; the error of an
    iteration is the MEAN of the items' relative errors (tensor.py:362-372) and convergence is decided once for all."""
    Bt, N = X.shape[0], X.dim() - 1

    def unf(n):
        return X.permute([0, n + 1] + list(range(1, n + 1)) + list(range(n + 2, N + 1))).reshape(Bt, X.shape[n + 1], -1)

    if init is not None:
        A = list(init)
    else:
        A = []
        for n in range(N):  # tensor.py:228-258
            g = unf(n)
            g = g @ _t(g)
            w, V = torch.linalg.eigh(g)
            reverse = torch.arange(w.shape[1] - 1, -1, -1)
            idx = torch.argsort(w)[:, reverse[:R]]
            c = V[[[i] for i in range(len(idx))], :, idx].transpose(-1, -2)
            if c.shape[2] < R:
                c = torch.cat((c, torch.randn(c.shape[0], c.shape[1], R - c.shape[2], dtype=c.dtype, device=c.device)), dim=2)
            A.append(c)
    xnorms = torch.sqrt(torch.sum(X**2, dim=list(range(1, X.dim()))))
    grams = [None] + [_t(A[n]) @ A[n] for n in range(1, N)]
    errors = []
    for it in range(max_iter):
        for n in range(N):
            khatri = torch.ones(Bt, 1, R, dtype=X.dtype, device=X.device)
            prod = torch.ones(Bt, R, R, dtype=X.dtype, device=X.device)
            for m in range(N - 1, -1, -1):
                if m != n:
                    prod *= grams[m]
                    khatri = torch.reshape(torch.einsum("bir,bjr->bijr", (A[m], khatri)), [Bt, -1, R])
            A[n] = _t(torch.linalg.lstsq(prod, _t(unf(n) @ khatri)).solution)
            grams[n] = _t(A[n]) @ A[n]
        acc = A[0]
        for c in A[1:]:
            acc = torch.einsum("bar,bir->bair", acc, c).reshape(Bt, -1, R)
        err = X - acc.sum(dim=2).reshape(X.shape)
        errors.append(float((torch.sqrt(torch.sum(err**2, dim=list(range(1, err.dim())))) / xnorms).mean()))
        if verbose:
            print("iter: {} | eps: {:.8f}".format(it, errors[-1]))
        if len(errors) >= 2 and errors[-2] - errors[-1] < tol:
            break
    return A, errors


# ---------------------------------------------------------------------------------------------- producers
def core_kron(a4: torch.Tensor, b4: torch.Tensor) -> torch.Tensor:
    """tensor.py:2309-2320 ``_core_kron`` (batch form) on [B, r, I, r'] cores."""
    c = a4[:, :, None, :, :, None] * b4[:, None, :, :, None, :]
    return c.reshape([a4.shape[0], a4.shape[1] * b4.shape[1], -1, a4.shape[-1] * b4.shape[-1]])


def scale(x: torch.Tensor, value) -> torch.Tensor:
    return x * value


def mm(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """[B, m, k] @ [B, k, n] (joins of integer-indexed slices, tensor.py:1114-1138, 1335-1345)."""
    return _mm(A, B)


def gather_chain(cores4: Sequence[torch.Tensor], idx: Sequence[torch.Tensor]) -> torch.Tensor:
    """Index-array block of tensor.py:1357-1378: cores [B, r_n, I_n, r_{n+1}] and one index vector per core ->
    [B, r_0, P, r_N], out[b, :, p, :] = prod_n cores[n][b, :, idx[n][p], :]."""
    X = cores4[0][:, :, idx[0], :]
    for c, i in zip(cores4[1:], idx[1:]):
        X = torch.einsum("biaj,bjak->biak", X, c[:, :, i, :])
    return X


def _maxvol_one(A: torch.Tensor, tol: float, max_iters: int):
    N, r = A.shape
    LU, piv = torch.linalg.lu_factor(A)  # getrf: the pivots of the reference's start (maxvol.py:138-145)
    index = torch.arange(N)
    for i, p in enumerate((piv[:r] - 1).tolist()):
        index[[i, p]] = index[[p, i]]
    U = torch.triu(LU[:r])
    L11 = torch.tril(LU[:r], -1) + torch.eye(r, dtype=A.dtype)
    C = torch.linalg.solve_triangular(U, A, upper=True, left=False)  # A = C L11 U
    C = torch.linalg.solve_triangular(L11, C, upper=False, left=False, unitriangular=True)
    iters = 0
    while True:
        q, p = divmod(int(torch.argmax(C.t().abs())), N)  # first maximum of |C^T| in row-major order
        if not abs(float(C[p, q])) > tol or iters >= max_iters:
            break
        index[q] = p
        x = C[p].clone()
        x[q] -= 1.0
        C.addr_(C[:, q] * (-1.0 / C[p, q]), x)  # C[n, k] += (alpha C[n, q]) x[k]
        iters += 1
    return index[:r].clone(), C


def maxvol(A3: torch.Tensor, tol: float, max_iters: int):
    """maxvol.py:115-170 on every item of [B, N, r] (N > r) -> index [B, r] int64, C [B, N, r]."""
    out = [_maxvol_one(a, tol, max_iters) for a in A3]
    return torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])


def minimize_step(e: torch.Tensor, Ra: int, I: int, Rb: int, lset: torch.Tensor, rset: torch.Tensor, best: torch.Tensor,
                  pos: torch.Tensor, flags: torch.Tensor) -> torch.Tensor:
    """Mirror of ttr_minimize_step, in place: e [Ra * I * Rb] <- pi/2 - atan(e - m0) in e's dtype, m0 = best if flags[0] (found)
    else 0; the state ``best`` (one element), ``pos`` (int64 [nl + 1 + nr]), ``flags`` (int32 [2]: found, invalid) is updated from
    the FIRST smallest entry of the original e (-0.0 == +0.0) where that is strictly smaller than ``best`` or nothing was found
    yet: pos = lset[a, 1:] ++ [i] ++ rset[c, :-1] for the entry (a I + i) Rb + c.  A non-finite entry sets flags[1] and leaves
    the rest of the state alone."""
    assert e.dim() == 1 and e.shape[0] == Ra * I * Rb and lset.shape[0] == Ra and rset.shape[0] == Rb
    found = bool(flags[0])
    orig = e.clone()
    m0 = best.reshape(()).clone() if found else torch.zeros((), dtype=e.dtype)
    e.copy_(math.pi / 2 - torch.atan(orig - m0))
    if not bool(torch.isfinite(orig).all()):
        flags[1] = 1
        return e
    v = orig.min()
    if found and not bool(v < best.reshape(())):
        return e
    m = int(torch.nonzero(orig == v)[0])
    a, i, c = m // (I * Rb), (m // Rb) % I, m % Rb
    best.reshape(-1)[0] = orig[m]
    flags[0] = 1
    pos.copy_(torch.cat([lset[a, 1:], torch.tensor([i], dtype=torch.int64), rset[c, : rset.shape[1] - 1]]))
    return e


def als_core(L: torch.Tensor, R: torch.Tensor, w: torch.Tensor, y: torch.Tensor, order: torch.Tensor, off: Sequence[int],
             I: int) -> torch.Tensor:
    """interpolation.py:71-90 with the design columns in (a, b) order: slice i of the new core [r0, I, r1] is the minimum-norm
    least-squares solution (gelsd) over the samples order[off[i]:off[i+1]], row k_p = w_p (L_p (x) R_p), k_p[a r1 + b] =
    w_p L_p[a] R_p[b], right-hand side w_p y_p.  A fresh tensor."""
    r0, r1 = L.shape[1], R.shape[1]
    core = torch.empty((r0, I, r1), dtype=L.dtype)
    for i in range(I):
        idx = order[off[i] : off[i + 1]]
        A = torch.reshape(L[idx, :, None] * R[idx, None, :], [len(idx), -1]) * w[idx, None]
        b = y[idx] * w[idx]
        sol = torch.linalg.lstsq(A, b[:, None], driver="gelsd").solution[:, 0]
        core[:, i, :] = torch.reshape(sol, (r0, r1))
    return core


def als_left_step(L: torch.Tensor, core: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """lefts[mu + 1] = lefts[mu] @ core[:, X[:, mu], :] (interpolation.py:84-87) on [P, r] interfaces."""
    return torch.einsum("pa,apb->pb", L, core[:, x, :])


def als_right_step(R: torch.Tensor, core: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """rights[mu - 1] = core[:, X[:, mu], :] @ rights[mu] (interpolation.py:67-70, 88-91) on [P, r] interfaces."""
    return torch.einsum("apb,pb->pa", core[:, x, :], R)


def sparse_canonical(X: torch.Tensor, shape: Sequence[int]):
    """The canonical sample order of ``sparse_tt_svd`` on the CPU: (perm, lev) with perm the lexicographic order (x_N major, x_1
    minor) and lev[p] the deepest mode, 1-based, in which sorted sample p differs from its predecessor (N for p = 0).  Raises
    ValueError for indices outside ``shape`` and for repeated positions."""
    P, N = X.shape
    if int(X.min()) < 0:
        raise ValueError("sparse_tt_svd: negative indices in X")
    for n in range(N):
        if int(X[:, n].max()) >= shape[n]:
            raise ValueError("sparse_tt_svd: index {} out of range for mode {} of size {}".format(int(X[:, n].max()), n, shape[n]))
    perm = torch.arange(P)
    for n in range(N):  # stable sorts, minor key first
        perm = perm[torch.sort(X[perm, n], stable=True).indices]
    Xs = X[perm]
    diff = Xs[1:] != Xs[:-1]
    lev = torch.full((P,), N, dtype=torch.int32)
    lev[1:] = (diff * torch.arange(1, N + 1)).max(dim=1).values.to(torch.int32)
    if P > 1 and int(lev[1:].min()) == 0:
        raise ValueError("sparse_tt_svd: repeated positions in X")
    return perm.to(torch.int32), lev


def sparse_step(V: torch.Tensor, I: int, colptr: torch.Tensor, blk_i: torch.Tensor, blkcol: torch.Tensor, delta: float,
                cap: int):
    """One step of interpolation.py:135-181 on a block table (V [nb, r]; column c owns the blocks colptr[c]:colptr[c+1], block b
    sits at mode index blk_i[b]): the dense D [r I, C] of ``sparse_covariance``, ``D D^T``, ``torch.linalg.eigh``, the
    reference's rank rule capped at ``cap``, and ``left^T D``.  Returns (left [r I, q], W [C, q] = (left^T D)^T)."""
    nb, r = V.shape
    C = colptr.shape[0] - 1
    D = torch.zeros(r * I, C, dtype=V.dtype)
    rows = torch.arange(r)[None, :] * I + blk_i.long()[:, None]
    D[rows, blkcol.long()[:, None].expand(nb, r)] = V
    w, v = torch.linalg.eigh(_mm(D, D.t()))
    w = torch.sqrt(torch.clamp(w, min=0)).flip(0)  # decreasing importance
    v = v.flip(1)
    tail = torch.cumsum((w**2).flip(0), dim=0)
    where = torch.where(tail <= delta**2)[0]
    kept = len(w) if len(where) == 0 else len(w) - 1 - int(where[-1])
    rank = max(1, min(cap, kept))
    left = v[:, :rank]
    return left, _mm(left.t(), D).t().contiguous()


# ---------------------------------------------------------------------------------------------- accepted inputs (automata.py:84-128)
ACCEPT_NEGATIVE, ACCEPT_SUM_MISMATCH, ACCEPT_BAD_INDEX = 1, 2, 4   # include/ttround_hip.h: TTR_ACCEPT_*


def accept_fibers(cores):
    """fibers[mu] = core_mu x_3 right_{mu+1} (fp64 [r_mu, I_mu]), right_mu = sum_i fibers[mu][:, i], right_N = 1, and the total
    right_0 (fp64 [r_0])."""
    right = torch.ones((cores[-1].shape[2], 1), dtype=torch.float64, device=cores[0].device)
    fibers = []
    for c in reversed(cores):
        r, I, rn = c.shape
        f = (c.double().reshape(r * I, rn) @ right).reshape(r, I)
        fibers.append(f)
        right = f.sum(dim=1, keepdim=True)
    return fibers[::-1], right[:, 0]


def accept_count(L: torch.Tensor, fiber: torch.Tensor) -> torch.Tensor:
    """Mirror of ttr_accept_count: C = rint(L @ fiber) in fp64, saturated at +-2^53, int64 [P, I]."""
    v = torch.round(L.double() @ fiber.double())
    v = torch.nan_to_num(v, nan=-2.0 ** 53).clamp(-2.0 ** 53, 2.0 ** 53)
    return v.to(torch.int64)


def accept_expand(L, core, C, childoff, cnt, idx, Xs, mu, flag, last):
    """Mirror of ttr_accept_expand, level-synchronous: every listed child (p, i) = divmod(idx[k], I) at once.  Returns
    (Lnew [K, r'] fp64 or None when ``last``, offnew [K], cntnew [K]); fills Xs[:, mu] and ORs ``flag`` (int32 [1])."""
    P, I = C.shape
    bits = 0
    if bool((C < 0).any()):
        bits |= ACCEPT_NEGATIVE
    if bool((C.sum(dim=1) != cnt).any()):
        bits |= ACCEPT_SUM_MISMATCH
    ok = (idx >= 0) & (idx < P * I)
    if not bool(ok.all()):
        bits |= ACCEPT_BAD_INDEX
    flag |= bits
    K, S = idx.shape[0], Xs.shape[0]
    pos = idx.clamp(0, P * I - 1)
    p, i = torch.div(pos, I, rounding_mode="floor"), pos % I
    offnew, cntnew = childoff.reshape(-1)[pos], C.reshape(-1)[pos]
    Lnew = None
    if not last:
        # [K, r] x [K, r, r'] as one product per symbol: the slices core[:, i, :] are shared by every slot of that symbol
        Lnew = torch.zeros((K, core.shape[2]), dtype=torch.float64, device=L.device)
        cd = core.double()
        for sym in range(I):
            sel = torch.nonzero(i == sym).reshape(-1)
            if sel.numel():
                Lnew[sel] = L[p[sel]].double() @ cd[:, sym, :]
    if K > 0 and S > 0:
        rows = torch.arange(S, device=Xs.device)
        k = (torch.searchsorted(offnew, rows, right=True) - 1).clamp(0, K - 1)   # the last slot with offnew[k] <= s
        Xs[:, mu] = i[k]
    return Lnew, offnew, cntnew


# ---------------------------------------------------------------------------------------------- sampling (tools.py:362-407)
SAMPLE_ZERO_TOTAL, SAMPLE_NONFINITE, SAMPLE_BAD_THRESHOLD = 1, 2, 4   # include/ttround_hip.h: TTR_SAMPLE_*


def sample_max_rank():
    """The host mirror has no rank limit."""
    return None


def _sample_fibers(cores, matvec):
    right = torch.ones((cores[-1].shape[2],), dtype=cores[0].dtype, device=cores[0].device)
    fibers = []
    for c in reversed(cores):
        r, I, rn = c.shape
        f = matvec(c.reshape(r * I, rn), right).reshape(r, I)
        fibers.append(f)
        right = f.sum(dim=1)
        # any positive scale of a right vector cancels in the comparison with u T; a zero vector stays zero (and is flagged)
        right = right / right.abs().max().clamp_min(torch.finfo(right.dtype).tiny)
    return fibers[::-1]


def sample_fibers(cores):
    """fibers[mu] = core_mu x_3 right_{mu+1} ([r_mu, I_mu], the cores' dtype), right_N = 1 and right_mu = sum_i fibers[mu][:, i]
    divided by its largest magnitude."""
    return _sample_fibers(cores, lambda A, v: A @ v)


def sample_step(L, fiber, core, u, x, flag, last):
    """Mirror of ttr_sample_step with the same definition: q = |L @ fiber| in the dtype, the running sum c and T in fp64,
    x[p] = the first i with c_i > u[p] T[p] (where rounding leaves none, the last i with q > 0), Lnew = (L @ core[:, x, :]) / T
    rounded once.  Fills ``x`` (a column of Xs), ORs ``flag`` (int32 [1]); a flagged sample gets x = -1 and a zero row.  Returns
    Lnew [P, r'] or None when ``last``."""
    P, I = L.shape[0], fiber.shape[1]
    q = (L @ fiber).abs().double()
    c = torch.cumsum(q, dim=1)
    T = c[:, -1]
    first = (c <= (u * T)[:, None]).sum(dim=1)             # c is non-decreasing: the number of c_i <= u T
    lastpos = ((q > 0) * torch.arange(1, I + 1, device=q.device)).amax(dim=1) - 1
    xi = torch.where(first < I, first, lastpos)
    bad_u = ~((u >= 0) & (u < 1))
    zero = T == 0
    nonfinite = ~torch.isfinite(T)
    flagged = bad_u | zero | nonfinite | (xi < 0)
    bits = ((SAMPLE_BAD_THRESHOLD if bool(bad_u.any()) else 0) | (SAMPLE_ZERO_TOTAL if bool(zero.any()) else 0)
            | (SAMPLE_NONFINITE if bool(nonfinite.any()) else 0))
    flag |= bits
    xi = torch.where(flagged, torch.full_like(xi, -1), xi)
    x.copy_(xi)
    if last:
        return None
    G = core[:, xi.clamp_min(0), :]                                     # [r, P, r']
    Lnew = (torch.einsum("pa,apb->pb", L, G).double() / T[:, None]).to(L.dtype)
    return torch.where(flagged[:, None], torch.zeros_like(Lnew), Lnew)


# ---------------------------------------------------------------------------------------------- TT / CP matrix products (matrix.py:420-468)
def tt_matvec_chain(cores: Sequence[torch.Tensor], x2d: torch.Tensor) -> torch.Tensor:
    """x2d [b, prod I_k] times the TT-matrix with the cores G_k [r_k, I_k, O_k, r_{k+1}] (r_0 = r_d = 1) -> [b, prod O_k]: the
    chain of ttr_ttm_step in torch ops.  X_0 = x2d^T read as [I_0, D_0, 1]; step k contracts (i, r) of X_k [I_k, D_k, r_k] with
    G_k and its output [D_k, O_k, r_{k+1}], row-major, is X_{k+1} [I_{k+1}, D_{k+1}, r_{k+1}]: a reshape, never a copy."""
    b = x2d.shape[0]
    X = x2d.t().contiguous()
    for G in cores:
        R, I = G.shape[0], G.shape[1]
        X = torch.einsum("idr,rios->dos", X.reshape(I, -1, R), G)
    return X.reshape(b, -1)


def ttm_step(X: torch.Tensor, G: torch.Tensor) -> torch.Tensor:
    """Y[dd, o, s] = sum_{i, r} X[i, dd, r] G[r, i, o, s] (ttr_ttm_step): X [I, D, R], G [R, I, O, S] -> Y [D, O, S]."""
    return torch.einsum("idr,rios->dos", X, G).contiguous()


def ttm_grad_input(dY: torch.Tensor, G: torch.Tensor) -> torch.Tensor:
    """dX[i, dd, r] = sum_{o, s} dY[dd, o, s] G[r, i, o, s] (ttr_ttm_grad_input): dY [D, O, S], G [R, I, O, S] -> dX [I, D, R]."""
    return torch.einsum("dos,rios->idr", dY, G).contiguous()


def ttm_grad_core(X: torch.Tensor, dY: torch.Tensor) -> torch.Tensor:
    """dG[r, i, o, s] = sum_dd X[i, dd, r] dY[dd, o, s] (ttr_ttm_grad_core): X [I, D, R], dY [D, O, S] -> dG [R, I, O, S]."""
    return torch.einsum("idr,dos->rios", X, dY).contiguous()


def cp_matvec_chain(cores: Sequence[torch.Tensor], x2d: torch.Tensor) -> torch.Tensor:
    """x2d [b, prod I_k] times the CP-matrix with the cores C_k [I_k, O_k, R] -> [b, prod O_k]: the chain of ttr_cpm_step in
    torch ops (the rank index is carried, step 0 broadcasts X_0 over it), then the sum over the rank."""
    b = x2d.shape[0]
    X = x2d.t().contiguous()
    for k, C in enumerate(cores):
        I, R = C.shape[0], C.shape[2]
        Xk = X.reshape(I, -1, 1) if k == 0 else X.reshape(I, -1, R)
        X = (Xk[:, :, None, :] * C[:, None, :, :]).sum(dim=0)
    return X.sum(dim=-1).reshape(b, -1)


# ---------------------------------------------------------------------------------------------- TT-matrix row lookup (lookup.py)
def lookup_digits(cores: Sequence[torch.Tensor], rows1d: torch.Tensor) -> torch.Tensor:
    """The int64 [P, d] digit table of the rows: row j (negative: j + rows) splits row-major over the input modes, i_1 most
    significant.  Digits 2 .. d are reduced modulo their mode; the FIRST is not, so a row outside [-rows, rows) shows as a first
    digit outside 0 .. I_1 - 1 (below 0 for a row below -rows) and nowhere else."""
    sizes = [int(c.shape[1]) for c in cores]
    total = 1
    for n in sizes:
        total *= n
    j = rows1d.to(torch.int64)
    j = torch.where(j < 0, j + total, j)
    cols, below = [], total
    for k, n in enumerate(sizes):
        below //= n
        q = torch.div(j, below, rounding_mode="floor")
        cols.append(q if k == 0 else q % n)
    return torch.stack(cols, dim=1)


def tt_lookup_chain(cores: Sequence[torch.Tensor], rows1d: torch.Tensor) -> torch.Tensor:
    """Rows ``rows1d`` [P] of the TT-matrix with the cores G_k [r_k, I_k, O_k, r_{k+1}] (r_0 = r_d = 1) -> [P, prod O_k]: the
    chain of ttr_ttm_lookup_step in torch ops.  Z_1 = G_1[0, i_1] [P, O_1, r_1]; step k contracts r of Z_{k-1} [P, D, r] with
    the slice G_k[:, i_k(p)] of every sample, and its output [P, D, O_k, r_k], row-major, is Z_k [P, D O_k, r_k].  Plain torch, so
    differentiable in the cores.  IndexError for a row outside [-rows, rows)."""
    P = rows1d.shape[0]
    digits = lookup_digits(cores, rows1d)
    i1 = digits[:, 0]
    if bool(((i1 < 0) | (i1 >= cores[0].shape[1])).any()):
        raise IndexError("tt_lookup: a row index lies outside the matrix")
    Z = cores[0][0][i1]                                            # [P, O_1, r_1]
    for k in range(1, len(cores)):
        Gk = cores[k][:, digits[:, k]]                             # [R, P, O, S]
        Z = torch.einsum("pdr,rpos->pdos", Z, Gk).reshape(P, -1, Gk.shape[3])
    return Z.reshape(P, -1)


def ttm_lookup_grad_core(X: torch.Tensor, xrow: Optional[torch.Tensor], dY: torch.Tensor, idx: torch.Tensor, I: int) -> torch.Tensor:
    """Mirror of ttr_ttm_lookup_grad_core: X [rows_x, D, R], dY [P, D, O, S], idx [P] (wrapped) -> dG [R, I, O, S],
    dG[r, i, o, s] = sum_{p: idx[p] = i} sum_dd X[xrow[p], dd, r] dY[p, dd, o, s]; a slice without samples is zero."""
    Xg = X if xrow is None else X[xrow]
    v = torch.remainder(idx.to(torch.int64), I)
    dG = torch.zeros((X.shape[2], I, dY.shape[2], dY.shape[3]), dtype=X.dtype, device=X.device)
    return dG.index_add_(1, v, torch.einsum("pdr,pdos->rpos", Xg, dY))


def ttm_lookup_grad_input(dY: torch.Tensor, G: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """Mirror of ttr_ttm_lookup_grad_input: dY [P, D, O, S], G [R, I, O, S], idx [P] (wrapped) -> dX [P, D, R],
    dX[p, dd, r] = sum_{o, s} dY[p, dd, o, s] G[r, idx[p], o, s]."""
    v = torch.remainder(idx.to(torch.int64), G.shape[1])
    return torch.einsum("pdos,rpos->pdr", dY, G[:, v])


def segment_sum(Y: torch.Tensor, seg: torch.Tensor, w: Optional[torch.Tensor] = None, perm: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Mirror of ttr_segment_sum: Y [P, C], seg [B + 1] (non-decreasing in 0 .. P) -> out [B, C], out[b] = the sum over
    q = seg[b] .. seg[b + 1] - 1 of (w[src(q)] or 1) Y[src(q)], src(q) = perm[q] (or q).  An ``index_add_``: differentiable in Y
    and w; an empty segment gives zeros."""
    P, B = Y.shape[0], seg.shape[0] - 1
    q = torch.arange(P, device=Y.device)
    bag = torch.searchsorted(seg[1:].contiguous(), q, right=True)      # the segment of position q; B at and past seg[B]
    live = (q >= seg[0]) & (bag < B)
    src = q if perm is None else perm
    rows = Y[src] if w is None else Y[src] * w[src][:, None]
    out = torch.zeros((B, Y.shape[1]), dtype=Y.dtype, device=Y.device)
    return out.index_add_(0, bag[live], rows[live])


# ---------------------------------------------------------------------------------------------- tt_solve (ttsolve.py)
def gemm2d(A: torch.Tensor, B: torch.Tensor, transA: bool = False, transB: bool = False) -> torch.Tensor:
    return (A.t() if transA else A) @ (B.t() if transB else B)


def env_half_apply(Phi: torch.Tensor, X: torch.Tensor, G: torch.Tensor) -> torch.Tensor:
    """Mirror of ttr_env_half_apply: Phi [R, A, R'], X [R', J, S'], G [A, I, J, A'] -> H [R, I, A', S'],
    H[r, i, c, s] = sum_{a, j} G[a, i, j, c] sum_b Phi[r, a, b] X[b, j, s]."""
    return torch.einsum("rab,bjs,aijc->rics", Phi, X, G).contiguous()


env_half_apply_unfused = env_half_apply


def local_matvec(Phi: torch.Tensor, G: torch.Tensor, Psi: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """y[r, i, s] = sum Phi[r, a, b] G[a, i, j, c] Psi[s, c, t] v[b, j, t]."""
    return torch.einsum("rics,tcs->rit", env_half_apply(Phi, v, G), Psi)


def env_update(side: str, env: torch.Tensor, G: torch.Tensor, bra: torch.Tensor, ket: torch.Tensor) -> torch.Tensor:
    """The interface of (bra, G, ket) moved over one site: "left" Phi [R, A, R'] -> [S, A', S'], "right" Psi [S, A', S'] ->
    [R, A, R'] (the mirrored operands)."""
    if side == "left":
        return torch.einsum("rit,rics->tcs", bra, env_half_apply(env, ket, G))
    if side != "right":
        raise ValueError("env_update: side must be 'left' or 'right'")
    H = env_half_apply(env, ket.permute(2, 1, 0), G.permute(3, 1, 2, 0))   # [s, i, a, r']
    return torch.einsum("ris,siab->rab", bra, H)


# ---------------------------------------------------------------------------------------------- tt_eigsh (tteigs.py)
# Mirror of ttr_ritz.hip: one Rayleigh-Ritz step of a three-vector LOBPCG on the vectors X, AX, W, AW, P, AP, written without a
# branch on a value, so that the same code on device tensors is the torch baseline of tools/eigs_bench.py.
RITZ_INIT, RITZ_STEP = 0, 1
RITZ_SA, RITZ_LA = 0, 1
RITZ_DROP = 64      # directions of the scaled Gram matrix below RITZ_DROP eps (of the vectors' dtype) of its largest eigenvalue go


def ritz_parts(dtype: torch.dtype, n: int) -> int:
    """The rows of ``part``: the mirror sums in one piece."""
    return 1


def ritz_workspace_bytes(dtype: torch.dtype, n: int) -> int:
    return 12 * 8 * ritz_parts(dtype, n)


def ritz_gram(mode: int, X, AX, W=None, AW=None, P=None, AP=None) -> torch.Tensor:
    """part [1, 12] in fp64: S = V^T V (xx, xw, xp, ww, wp, pp) and T = V^T A V (x.ax, x.aw, x.ap, w.aw, w.ap, p.ap) of
    V = [X W P]; RITZ_INIT fills only S_xx and T_xx, a P of None counts as zeros."""
    d = lambda a, b: torch.dot(a.reshape(-1).double(), b.reshape(-1).double())  # noqa: E731
    zero = torch.zeros((), dtype=torch.float64, device=X.device)
    if mode == RITZ_INIT:
        vals = [d(X, X)] + [zero] * 5 + [d(X, AX)] + [zero] * 5
    else:
        hasp = P is not None
        vals = [d(X, X), d(X, W), d(X, P) if hasp else zero, d(W, W), d(W, P) if hasp else zero, d(P, P) if hasp else zero,
                d(X, AX), d(X, AW), d(X, AP) if hasp else zero, d(W, AW), d(W, AP) if hasp else zero, d(P, AP) if hasp else zero]
    return torch.stack(vals).reshape(1, 12)


def _sym3(v):
    """The symmetric 3 x 3 matrix of its upper triangle (00, 01, 02, 11, 12, 22)."""
    return torch.stack([v[0], v[1], v[2], v[1], v[3], v[4], v[2], v[4], v[5]]).reshape(3, 3)


def ritz_pencil(S: torch.Tensor, T: torch.Tensor, which: int, eps: float):
    """The extreme Ritz pair of the 3 x 3 pencil (T, S) in fp64 -> (c [3], theta, kept, relgap).  S is scaled to unit diagonal
    (a zero diagonal drops the direction), the eigendirections of the scaled S below ``RITZ_DROP eps`` of its largest eigenvalue
    are dropped, and the whitened problem is solved; c is scaled to c^T S c = 1 with c[0] >= 0, theta = c^T T c.  ``relgap`` is
    the gap between the chosen Ritz value and the next, over the spread of the kept ones (1 when one direction is kept)."""
    d = torch.diagonal(S)
    ok = d > 0
    dinv = torch.where(ok, torch.where(ok, d, torch.ones_like(d)).rsqrt(), torch.zeros_like(d))
    Ss = S * dinv[:, None] * dinv[None, :]
    Ts = T * dinv[:, None] * dinv[None, :]
    mu, Q = torch.linalg.eigh(Ss)
    keep = mu > (RITZ_DROP * eps) * mu.max()
    w = torch.where(keep, torch.where(keep, mu, torch.ones_like(mu)).rsqrt(), torch.zeros_like(mu))
    Z = Q * w[None, :]
    M = Z.t() @ Ts @ Z
    if which == RITZ_LA:
        M = -M
    M = (M + M.t()) / 2
    big = 2.0 * (M.abs().sum() + 1.0)
    M = M + torch.diag(torch.where(keep, torch.zeros_like(mu), big.expand(3)))      # the dropped directions: never the smallest
    lam, Y = torch.linalg.eigh(M)
    c = dinv * (Z @ Y[:, 0])
    c = c / torch.sqrt(c @ S @ c)
    c = torch.where(c[0] < 0, -c, c)
    theta = c @ T @ c
    kept = keep.sum()
    top = torch.where(torch.arange(3, device=S.device) < kept, lam, lam[0]).max()
    relgap = torch.where(top > lam[0], (lam[1] - lam[0]) / torch.where(top > lam[0], top - lam[0], torch.ones_like(top)),
                         torch.ones_like(top))
    return c, theta, kept, relgap


def ritz_update(mode: int, which: int, first: int, rel: float, part: torch.Tensor, X, AX, W, AW, P, AP, state: torch.Tensor,
                sweep: torch.Tensor) -> None:
    """Mirror of ttr_ritz_update, in place.  The partial sums are added in the order of their rows; the pencil is solved in fp64
    (``ritz_pencil``); the vectors are updated in fp64 and rounded once, W = AX - theta X from the ROUNDED new X and AX.
    RITZ_INIT: X and AX are divided by ||X||, W is set, P and AP are zeroed.  RITZ_STEP: X <- c0 X + Pn, AX <- c0 AX + APn,
    P <- Pn = c1 W + c2 P, AP <- APn; a P of None is a zero that is neither read nor written.  A frozen step (res <= rel) or a
    flagged one (1: a non-finite sum, 2: S_xx == 0) writes no vector and solves no pencil (c = (1, 0, 0), kept = 0).  state (fp64[8]) = theta', res, frozen, flags, c0, c1,
    c2, kept; sweep (fp64[4]): [0] = max([0], res) when ``first``, [1] += (flags != 0), [2] = theta', [3] |= flags."""
    dt = X.dtype
    g = part[0].clone()
    for r in range(1, part.shape[0]):
        g = g + part[r]
    S, T = _sym3(g[:6]), _sym3(g[6:])
    finite = torch.isfinite(g).all()
    sxx = torch.where(finite, g[0], torch.ones_like(g[0]))
    flags = torch.where(finite, torch.zeros_like(sxx), torch.ones_like(sxx)) + torch.where(sxx == 0, 2.0, 0.0).to(sxx.dtype)
    good = flags == 0
    sxx = torch.where(good, sxx, torch.ones_like(sxx))
    one, zero = torch.ones_like(sxx), torch.zeros_like(sxx)
    if mode == RITZ_INIT:
        inv = sxx.rsqrt()
        theta = torch.where(good, g[6] / sxx, zero)
        res, frozen, kept = zero, zero, torch.where(good, one, zero)     # a flagged step keeps no direction
        c = torch.stack([torch.where(good, inv, one), zero, zero])
        Xn = (X.double() * c[0]).to(dt)
        AXn = (AX.double() * c[0]).to(dt)
        Wn = (AXn.double() - theta * Xn.double()).to(dt)
        X.copy_(Xn)
        AX.copy_(AXn)
        W.copy_(torch.where(good, Wn, W))
        if P is not None:
            P.copy_(torch.where(good, torch.zeros_like(P), P))
            AP.copy_(torch.where(good, torch.zeros_like(AP), AP))
    else:
        theta0 = g[6] / sxx
        sww = g[3]
        res = torch.where(sww > 0, torch.sqrt(sww / torch.where(sww > 0, sww + theta0 * theta0 * sxx, one)), zero)
        res = torch.where(good, res, zero)
        frozen = torch.where(good & (res <= rel), one, zero)
        eye = torch.eye(3, dtype=S.dtype, device=S.device)
        c, theta, kept, _ = ritz_pencil(torch.where(good, S, eye), torch.where(good, T, eye), which, float(torch.finfo(dt).eps))
        act = good & (frozen == 0)
        theta = torch.where(act, theta, torch.where(good, theta0, zero))
        c = torch.where(act, c, torch.stack([one, zero, zero]))
        kept = torch.where(act, kept.to(sxx.dtype), zero)            # a frozen or flagged step solves no pencil
        Pn = c[1] * W.double() + (c[2] * P.double() if P is not None else 0.0)
        APn = c[1] * AW.double() + (c[2] * AP.double() if P is not None else 0.0)
        Xn = (c[0] * X.double() + Pn).to(dt)
        AXn = (c[0] * AX.double() + APn).to(dt)
        Wn = (AXn.double() - theta * Xn.double()).to(dt)
        X.copy_(torch.where(act, Xn, X))
        AX.copy_(torch.where(act, AXn, AX))
        W.copy_(torch.where(act, Wn, W))
        if P is not None:
            P.copy_(torch.where(act, Pn.to(dt), P))
            AP.copy_(torch.where(act, APn.to(dt), AP))
    state.copy_(torch.stack([theta, res, frozen, flags, c[0], c[1], c[2], kept.to(sxx.dtype)]))
    if first:
        sweep[0:1].copy_(torch.maximum(sweep[0:1], res.reshape(1)))
    sweep[1:2].add_((flags != 0).to(sweep.dtype).reshape(1))
    sweep[2:3].copy_(theta.reshape(1))
    sweep[3:4].copy_(torch.where((sweep[3:4] == flags) | (flags == 0), sweep[3:4], torch.where(sweep[3:4] == 0, flags, 3.0 * one)).reshape(1))


# ---------------------------------------------------------------------------------------------- tt_amen_solve (ttamen.py)
# Mirror of ttr_cg.hip: one conjugate-gradient step in three calls on the vectors v, r, p, Bp, with the scalars in an fp64 state
# of 8 words (rs slot 0, rs slot 1, thr2, bad, live, alpha, pBp, beta; include/ttround_hip.h).  Written without a branch on a value,
# so that the same code on device tensors is the torch baseline of tools/amen_bench.py.
def cg_parts(dtype: torch.dtype, n: int) -> int:
    """The columns of ``part``: the mirror sums in one piece."""
    return 1


def cg_workspace_bytes(dtype: torch.dtype, n: int) -> int:
    return 2 * 8 * cg_parts(dtype, n)


def _row_sum(row: torch.Tensor) -> torch.Tensor:
    s = row[0].clone()
    for g in range(1, row.shape[0]):
        s = s + row[g]
    return s


def cg_dot(p: torch.Tensor, Bp: torch.Tensor, part: torch.Tensor) -> None:
    """part[0] (of an fp64 [2, parts]) = the shares of p . Bp in fp64: here one share, the rest zeros."""
    part[0].zero_()
    part[0, 0:1].copy_(torch.dot(p.double(), Bp.double()).reshape(1))


def cg_update(step: int, p: torch.Tensor, Bp: torch.Tensor, v: torch.Tensor, r: torch.Tensor, part: torch.Tensor,
              state: torch.Tensor) -> None:
    """Mirror of ttr_cg_update, in place.  pBp is the sum of part[0] in the order of its entries; with rs = state[step & 1] and
    thr2 = state[2]: live = (rs > thr2) & (pBp > 0), alpha = rs / pBp where live, else 0; v += alpha p and r -= alpha Bp in fp64,
    rounded once, only where live; part[1] = the shares of r . r of the rounded r (zeros where not live); state[3] += 1 for an
    active step with pBp <= 0, state[4:7] = live, alpha, pBp."""
    dt, slot = v.dtype, int(step) & 1
    pBp = _row_sum(part[0])
    rs, thr2 = state[slot], state[2]
    one, zero = torch.ones_like(pBp), torch.zeros_like(pBp)
    active, good = rs > thr2, pBp > 0
    live = active & good
    alpha = torch.where(live, rs / torch.where(good, pBp, one), zero)
    vn = torch.addcmul(v.double(), p.double(), alpha).to(dt)
    rn = torch.addcmul(r.double(), Bp.double(), -alpha).to(dt)
    v.copy_(torch.where(live, vn, v))
    r.copy_(torch.where(live, rn, r))
    part[1].zero_()
    part[1, 0:1].copy_(torch.where(live, torch.dot(rn.double(), rn.double()), zero).reshape(1))
    state[3:4].add_((active & ~good).to(state.dtype).reshape(1))
    state[4:7].copy_(torch.stack([live.to(state.dtype), alpha, pBp]))


def cg_direction(step: int, r: torch.Tensor, p: torch.Tensor, part: torch.Tensor, state: torch.Tensor) -> None:
    """Mirror of ttr_cg_direction, in place.  rs' is the sum of part[1]; where the step was live (state[4]):
    beta = rs' / max(rs, tiny of the dtype), p = r + beta p in fp64, rounded once, and the other rs slot takes rs'; where it was
    not, p stays, beta = 0 and the slot takes rs.  state[7] = beta."""
    dt, slot = p.dtype, int(step) & 1
    rsn = _row_sum(part[1])
    rs = state[slot]
    live = state[4] != 0
    zero = torch.zeros_like(rs)
    beta = torch.where(live, rsn / rs.clamp_min(float(torch.finfo(dt).tiny)), zero)
    pn = torch.addcmul(r.double(), p.double(), beta).to(dt)
    p.copy_(torch.where(live, pn, p))
    state[1 - slot:2 - slot].copy_(torch.where(live, rsn, rs).reshape(1))
    state[7:8].copy_(beta.reshape(1))


def cg_solve(Phi, Ak, Psi, f, x0, rel: float, iters: int, stat: torch.Tensor) -> torch.Tensor:
    """The local solve of tt_amen_solve on the CPU: ``ttsolve._cg`` itself, the specification of the kernels."""
    import sys

    from .ttsolve import _cg

    return _cg(sys.modules[__name__], Phi, Ak, Psi, f, x0, rel, iters, stat)

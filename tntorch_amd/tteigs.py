"""``tt_eigsh``: the smallest or largest eigenvalue of a symmetric ``TTMatrix`` with its eigenvector as a train, by one-site ALS
with fixed ranks (one-site DMRG).  Nothing dense is formed.

With every core of ``x`` but core ``k`` orthogonalised towards site ``k``, the Rayleigh quotient ``x^T A x / x^T x`` over that
core is the one of the small symmetric matrix ``B_k`` of ``ttsolve.py``, which is never formed: ``ops.local_matvec`` applies it.
The local eigensolver is a three-vector LOBPCG without a preconditioner on six vectors ``X, AX, W, AW, P, AP`` of ``R I S``
elements.  One step is four launches whatever the size: the two of the matvec ``AW = B_k W``, and

    ritz_gram      the twelve sums of S = V^T V and T = V^T A V, V = [X W P], as fp64 partials per workgroup
    ritz_update    adds the partials in a fixed order, solves the 3 x 3 pencil (T, S) in fp64 and updates the six vectors

The step count is fixed and nothing is read back inside a sweep: a system whose residual ``||W|| / ||AX||`` is ``<= tol / 10``
is frozen, its steps write nothing.  One readback per sweep fetches the largest residual the sites had before their solves, the
count of flagged steps and the latest Ritz value.

Not here: several eigenpairs at once (block LOBPCG or deflation), rank adaptation, a preconditioner, interior eigenvalues, a
single-launch path for small local problems, batched operands, the device backward.
"""

from __future__ import annotations

import math
from typing import List, Optional

import torch

from ._dispatch import ops_for
from .tensor import Tensor, _not_in_scope
from .ttalgebra import _check_operands, _matrix_cores, _refuse_device_grad, tt_apply, tt_transpose
from .ttsolve import _max_ranks, _tt_norm

__all__ = ["tt_eigsh"]

# how often the driver has read device scalars back, by kind ("sweep": the stopping value, the flag count and theta in one small
# tensor, once per sweep; "residual": the final residual of return_info).  Tests read it; nothing else does.
READBACKS = {"sweep": 0, "residual": 0}


def _read(kind: str, t: torch.Tensor) -> List[float]:
    READBACKS[kind] += 1
    return [float(v) for v in t.detach().cpu().reshape(-1).tolist()]


def _lobpcg(ops, Phi, Ak, Psi, x0, which: int, rel: float, iters: int, state: torch.Tensor, sweep: torch.Tensor) -> torch.Tensor:
    """``iters`` steps of three-vector LOBPCG on B v = theta v from the core x0, with no readback; returns the normalised core.
    sweep[0] takes the maximum with the residual x0 had, sweep[1] counts the flagged steps, sweep[2] is the latest theta."""
    shape = x0.shape
    X = x0.clone().reshape(-1)
    AX = ops.local_matvec(Phi, Ak, Psi, x0).contiguous().reshape(-1)
    n = X.numel()
    W, P, AP = torch.zeros((3, (n + 3) // 4 * 4), dtype=X.dtype, device=X.device)[:, :n].unbind(0)   # rows 16 bytes aligned
    ops.ritz_update(ops.RITZ_INIT, which, 0, rel, ops.ritz_gram(ops.RITZ_INIT, X, AX), X, AX, W, None, P, AP, state, sweep)
    for it in range(iters):
        AW = ops.local_matvec(Phi, Ak, Psi, W.reshape(shape)).contiguous().reshape(-1)
        part = ops.ritz_gram(ops.RITZ_STEP, X, AX, W, AW, P if it else None, AP if it else None)     # (P = 0 in the first step)
        ops.ritz_update(ops.RITZ_STEP, which, int(it == 0), rel, part, X, AX, W, AW, P, AP, state, sweep)
    return X.reshape(shape)


def tt_eigsh(tt_matrix, x0: Optional[Tensor] = None, ranks_tt=None, which: str = "SA", nswp: int = 20, tol=None,
             local_iters: int = 50, verbose: bool = False, return_info: bool = False):
    """``(value, x)``: the smallest (``which="SA"``) or largest (``"LA"``) algebraic eigenvalue of the symmetric ``tt_matrix``
    and a train ``x`` with ``||x|| = 1`` and ``tn.tt_apply(tt_matrix, x) ~ value x``.  ``value`` is a 0-dim tensor on the cores'
    device in their dtype; the cores of ``x`` are orthonormal up to the last visited site.

    The matrix must be square in every mode and symmetric.  Symmetry is NOT checked; positive definiteness is not needed.

    One-site ALS with fixed ranks: those of ``x0`` if it is given (its cores are never written), else of
    ``tn.rand(shape, ranks_tt=ranks_tt)``, drawn on the CPU and moved to the matrix's device and dtype, the ranks capped at the
    largest the shape admits; one of the two is needed.  A sweep goes left to right and back.  Every local eigenproblem gets
    ``local_iters`` steps of a three-vector LOBPCG from the current core, frozen once its residual ``||B v - theta v|| / ||B v||``
    is ``<= tol / 10``; the largest residual the sites had BEFORE their solves is read back once per sweep, and the sweeps stop
    when it is ``<= tol`` or after ``nswp`` of them.  ``tol=None``: ``sqrt(eps)`` of the dtype (3.45e-4 in fp32, 1.49e-8 in
    fp64).  ``verbose`` prints one line per sweep.  Tucker factors of ``x0`` are contracted in.  With fixed ranks below the
    eigenvector's the value is variational: an upper bound of the smallest eigenvalue (a lower bound of the largest).

    ``return_info=True`` returns ``(value, x, info)`` with ``sweeps``, ``converged``, ``local_residuals`` (one float per sweep),
    ``values`` (theta after each sweep) and ``residual``, ``||A x - value x|| / ||A x||``, computed once at the end from
    ``tt_apply`` and the orthogonalised difference train.

    A zero ``x0`` and a non-finite value met in a sweep raise ``ValueError`` after that sweep's readback.  The call runs under
    ``torch.no_grad()`` and returns detached cores; on the device an operand that requires grad raises ``NotImplementedError``
    under grad mode."""
    who = "tt_eigsh"
    G = _matrix_cores(who, "the first argument", tt_matrix)
    N = len(G)
    if x0 is not None:
        if not isinstance(x0, Tensor):
            raise ValueError("{}: x0 must be a tntorch_amd.Tensor, got {}".format(who, type(x0).__name__))
        if x0.batch:
            raise ValueError("{}: batched tensors are not supported (x0)".format(who))
        if any(c.dim() == 2 for c in x0.cores):
            _not_in_scope("tt_eigsh with CP cores")
        if x0.dim() != N:
            raise ValueError("{}: the matrix has {} modes, x0 has {}".format(who, N, x0.dim()))
        if x0.cores[0].shape[0] != 1 or x0.cores[-1].shape[-1] != 1:
            raise ValueError("{}: the boundary ranks of x0 must be 1, got {} and {}".format(
                who, x0.cores[0].shape[0], x0.cores[-1].shape[-1]))
    for k, g in enumerate(G):
        if int(g.shape[1]) != int(g.shape[2]):
            raise ValueError("{}: mode {} of the matrix is not square: {} x {}".format(who, k, int(g.shape[1]), int(g.shape[2])))
        if x0 is not None and int(x0.shape[k]) != int(g.shape[1]):
            raise ValueError("{}: mode {} of x0 has size {}, the matrix's {}".format(who, k, int(x0.shape[k]), int(g.shape[1])))
    if x0 is None and ranks_tt is None:
        raise ValueError("{}: give x0 or ranks_tt (the ranks of the eigenvector are fixed)".format(who))
    if int(nswp) < 1 or int(local_iters) < 1:
        raise ValueError("{}: nswp and local_iters must be at least 1, got {} and {}".format(who, nswp, local_iters))
    if tol is not None and not float(tol) > 0:
        raise ValueError("{}: tol must be positive, got {}".format(who, tol))
    if which not in ("SA", "LA"):
        raise ValueError("{}: which must be 'SA' or 'LA', got {!r}".format(who, which))
    tensors = [] if x0 is None else list(x0.cores) + [U for U in x0.Us if U is not None]
    if _check_operands(who, G, tensors) and torch.is_grad_enabled():
        _refuse_device_grad(who)
    with torch.no_grad():
        return _eigsh(tt_matrix, x0, ranks_tt, which, int(nswp), tol, int(local_iters), verbose, return_info)


def _eigsh(tt_matrix, x0, ranks_tt, which, nswp, tol, local_iters, verbose, return_info):
    who = "tt_eigsh"
    M = type(tt_matrix)([g.detach() for g in tt_matrix.cores], None, tt_matrix.input_dims.tolist(), tt_matrix.output_dims.tolist())
    dtype, device = M.cores[0].dtype, M.cores[0].device
    N, shape = len(M.cores), [int(g.shape[1]) for g in M.cores]
    ops = ops_for(M.cores[0])
    A = tt_transpose(M).cores                                 # A_k [a, i, j, a'] with (A x)[i] = sum_j A[i, j] x[j], as in tt_solve
    tol = math.sqrt(torch.finfo(dtype).eps) if tol is None else float(tol)
    info = {"sweeps": 0, "converged": False, "local_residuals": [], "values": [], "residual": 0.0}

    if x0 is not None:
        x0 = Tensor([c.detach() for c in x0.cores], Us=[None if U is None else U.detach() for U in x0.Us])
        xs = [c.clone() for c in x0._absorbed4()]             # [1, r, n, s]
    else:
        from .create import rand

        want = list(ranks_tt) if hasattr(ranks_tt, "__len__") else [ranks_tt] * (N - 1)
        if len(want) != N - 1:
            raise ValueError("{}: ranks_tt needs {} entries, got {}".format(who, N - 1, len(want)))
        ranks = [max(1, min(int(r), cap)) for r, cap in zip(want, _max_ranks(shape))]
        start = rand(shape, ranks_tt=ranks) if N > 1 else rand(shape, ranks_tt=[])
        xs = [c.to(device=device, dtype=dtype)[None] for c in start.cores]

    one = lambda *s: torch.ones(s, dtype=dtype, device=device)  # noqa: E731
    for mu in range(N - 1, 0, -1):
        ops.right_orthogonalize(xs, mu)
    Phi: List[Optional[torch.Tensor]] = [None] * N
    Psi: List[Optional[torch.Tensor]] = [None] * N
    Phi[0], Psi[N - 1] = one(1, 1, 1), one(1, 1, 1)

    def move(side: str, k: int):
        xk = xs[k][0]
        if side == "left":
            Phi[k + 1] = ops.env_update("left", Phi[k], A[k], xk, xk)
        else:
            Psi[k - 1] = ops.env_update("right", Psi[k], A[k], xk, xk)

    for k in range(N - 1, 0, -1):
        move("right", k)

    state = torch.zeros(8, dtype=torch.float64, device=device)    # of the latest step (ritz_update)
    stat = torch.zeros(4, dtype=torch.float64, device=device)     # of the sweep: [largest first residual, flagged steps, theta, flag bits]
    wh = ops.RITZ_SA if which == "SA" else ops.RITZ_LA

    def solve(k: int):
        xs[k] = _lobpcg(ops, Phi[k], A[k], Psi[k], xs[k][0], wh, tol / 10.0, local_iters, state, stat)[None]

    for sweep in range(nswp):
        stat.zero_()
        if N == 1:
            solve(0)
        for k in range(N - 1):
            solve(k)
            ops.left_orthogonalize(xs, k)
            move("left", k)
        for k in range(N - 1, 0, -1):
            solve(k)
            ops.right_orthogonalize(xs, k)
            move("right", k)
        worst, bad, theta, bits = _read("sweep", stat)
        if bad > 0 or not (math.isfinite(worst) and math.isfinite(theta)):
            if int(bits) & 2:
                raise ValueError("{}: the start is the zero train (a local problem met a zero vector in sweep {})".format(who, sweep + 1))
            raise ValueError("{}: a non-finite value was met in sweep {}".format(who, sweep + 1))
        info["sweeps"] = sweep + 1
        info["local_residuals"].append(worst)
        info["values"].append(theta)
        if verbose:
            print("tt_eigsh: sweep {:3d}  value {:.12e}  largest local residual {:.3e}".format(sweep + 1, theta, worst))
        if worst <= tol:
            info["converged"] = True
            break

    value = stat[2].to(dtype).clone()
    x = Tensor([c[0] for c in xs])
    if not return_info:
        return value, x
    Ax = tt_apply(M, x)
    diff = Ax - Tensor([x.cores[0] * value] + list(x.cores[1:]))
    num = _tt_norm(ops, diff._absorbed4()).reshape(1)
    den = _tt_norm(ops, Ax._absorbed4()).reshape(1)
    r = _read("residual", torch.cat([num.double(), den.double()]))
    info["residual"] = r[0] / r[1] if r[1] > 0 else 0.0
    return value, x, info

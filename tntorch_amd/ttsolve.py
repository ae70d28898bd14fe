"""``tt_solve``: the train ``x`` with ``tt_apply(M, x) ~ b`` for a symmetric positive definite ``TTMatrix`` ``M`` and a
``Tensor`` ``b``, by one-site ALS with fixed ranks.  Nothing dense is formed.

With every core of ``x`` but core ``k`` orthogonalised towards site ``k``, minimising the energy ``x^T A x / 2 - b^T x`` over
that core is the small SPD system ``B_k v = f_k``:

    B_k v [r, i, s] = sum Phi_k[r, a, r'] A_k[a, i, j, a'] Psi_k[s, a', s'] v[r', j, s']        f_k = phi_k b_k psi_k

``Phi_k`` / ``Psi_k`` are the interfaces of (x, A, x) left / right of the site, ``phi_k`` / ``psi_k`` those of (x, b).  ``B_k`` is
never formed: conjugate gradients apply it, thousands of times per solve (sites x sweeps x iterations), and one application is

    H = env_half_apply(Phi_k, v, A_k)        [R, I, A', S']   ttr_env_half_apply: one launch, the middle intermediate stays on chip
    y = H [R I, A' S'] @ Psi_k [S, A' S']^T                   ttr_gemm on H as it lies

The same ``H`` with the new core in the place of ``v`` gives the next interface, ``Phi_{k+1} = core^T [S, R I] @ H`` (a second
ttr_gemm), and the right-to-left sweep runs the same kernel on the mirrored operands (rank-swapped views of ``A_k``, read where
they lie).  The algorithm stands here once, for both devices; the module of ``ops_for`` supplies ``env_half_apply``,
``local_matvec``, ``env_update``, ``gemm2d`` and the QR steps (``left_orthogonalize`` / ``right_orthogonalize``).

Conjugate gradients run with no host synchronisation: the iteration count is fixed, the scalars stay on the device, and a
system that has converged has its ``alpha`` forced to 0 so the remaining iterations change nothing.  One readback per sweep
fetches the largest local residual and the flag of a lost positive definiteness.

Not here: rank adaptation (AMEn enrichment is ``tt_amen_solve``, ttamen.py, which shares the checks and helpers below; two-site
DMRG), nonsymmetric local solvers (GMRES), a preconditioner for the local CG, a fused kernel for CG's vector updates (torch
does them here; ``tt_amen_solve`` has one), the variational ``tt_apply`` that the same kernel with bra != ket
would serve, eigenvalue solvers, batched operands and the device backward.
"""

from __future__ import annotations

import math
from typing import List, Optional

import torch

from ._dispatch import ops_for
from .tensor import Tensor, _not_in_scope
from .ttalgebra import _check_operands, _matrix_cores, _refuse_device_grad, tt_apply, tt_transpose

__all__ = ["tt_solve"]

# how often the driver has read device scalars back, by kind ("sweep": the stopping value and the flag, once per sweep;
# "setup": ||b||; "residual": the final residual of return_info).  Tests read it; nothing else does.
READBACKS = {"sweep": 0, "setup": 0, "residual": 0}


def _read(kind: str, t: torch.Tensor) -> List[float]:
    READBACKS[kind] += 1
    return [float(v) for v in t.detach().cpu().reshape(-1).tolist()]


def _max_ranks(shape: List[int]) -> List[int]:
    """The largest TT ranks a train of this shape can have: bond k is min(prod(shape[:k]), prod(shape[k:]))."""
    out = []
    for k in range(1, len(shape)):
        out.append(min(math.prod(shape[:k]), math.prod(shape[k:])))
    return out


def _rhs_local(ops, phi, bk, psi):
    """f[r, i, s] = sum phi[r, c] b[c, i, c'] psi[s, c']: two small GEMMs."""
    R, (C, I, C1), S = phi.shape[0], bk.shape, psi.shape[0]
    t = ops.gemm2d(phi, bk.reshape(C, I * C1)).reshape(R * I, C1)
    return ops.gemm2d(t, psi, transB=True).reshape(R, I, S)


def _rhs_update(ops, side, env, bk, xk):
    """The interface of (x, b) moved over one site: "left" phi [R, C] -> [S, C'], "right" psi [S, C'] -> [R, C]."""
    C, I, C1 = bk.shape
    R, _, S = xk.shape
    if side == "left":
        t = ops.gemm2d(env, bk.reshape(C, I * C1)).reshape(R * I, C1)
        return ops.gemm2d(xk.reshape(R * I, S), t, transA=True)
    u = ops.gemm2d(bk.reshape(C * I, C1), env, transB=True).reshape(C, I * S)
    return ops.gemm2d(xk.reshape(R, I * S), u, transB=True)


def _cg(ops, Phi, Ak, Psi, f, x0, rel: float, iters: int, stat: torch.Tensor) -> torch.Tensor:
    """``iters`` steps of conjugate gradients on B v = f from x0, down to ||r|| <= rel ||f||, with no readback.  stat[0] takes
    the maximum with the first relative residual ||B x0 - f|| / ||f||, stat[1] counts the steps with p^T B p <= 0."""
    shape = f.shape
    v = x0.clone().reshape(-1)
    fv = f.reshape(-1)
    r = fv - ops.local_matvec(Phi, Ak, Psi, x0).reshape(-1)
    p = r.clone()
    rs = torch.dot(r, r)
    fn2 = torch.dot(fv, fv)
    tiny = torch.finfo(f.dtype).tiny
    stat[0:1].copy_(torch.maximum(stat[0:1], torch.sqrt(rs / fn2.clamp_min(tiny)).reshape(1)))
    thr2 = (rel * rel) * fn2
    zero = torch.zeros((), dtype=f.dtype, device=f.device)
    for _ in range(iters):
        Bp = ops.local_matvec(Phi, Ak, Psi, p.reshape(shape)).reshape(-1)
        pBp = torch.dot(p, Bp)
        active = rs > thr2
        good = pBp > 0
        stat[1:2].add_((active & ~good).to(f.dtype).reshape(1))
        alpha = torch.where(active & good, rs / torch.where(good, pBp, torch.ones_like(pBp)), zero)
        v.add_(alpha * p)
        r.sub_(alpha * Bp)
        rs_new = torch.dot(r, r)
        beta = torch.where(active & good, rs_new / rs.clamp_min(tiny), zero)
        p = r + beta * p
        rs = rs_new
    return v.reshape(shape)


def _tt_norm(ops, cores4: List[torch.Tensor]) -> torch.Tensor:
    """||t|| of a train [1, r, n, s] by orthogonalising it to its last core: no cancellation between large terms."""
    c = list(cores4)
    for mu in range(len(c) - 1):
        ops.left_orthogonalize(c, mu)
    return ops.dense_norm(c[-1].contiguous())


def tt_solve(tt_matrix, b, transpose: bool = False, x0: Optional[Tensor] = None, ranks_tt=None, nswp: int = 20, tol=None,
             local_iters: int = 50, verbose: bool = False, return_info: bool = False):
    """The train ``x`` with ``tn.tt_apply(tt_matrix, x, transpose=transpose)`` approximately ``b``: by default the solution of
    ``vec(x) @ M = vec(b)``, with ``transpose=True`` of ``M @ vec(x) = vec(b)`` (``tt_multiply``'s convention; the transposed form
    reads ``tt_transpose`` views of the cores, nothing is copied).

    The matrix must be square in every mode (``input_dims[k] == output_dims[k] == b.shape[k]``) and symmetric positive definite.
    Symmetry is NOT checked (for a symmetric matrix the two forms coincide); a loss of positive definiteness is detected -- a
    local CG step with ``p^T B p <= 0`` -- and raises ``ValueError`` at the end of the sweep.  A nonsymmetric system is solved
    through its normal equations: ``tt_solve(tt_matmul(tt_transpose(A), A), tt_apply(A, b))`` for ``A @ vec(x) = vec(b)``.

    One-site ALS with fixed ranks: those of ``x0`` if it is given (its cores are never written), else of
    ``tn.rand(b.shape, ranks_tt=ranks_tt)``, drawn on the CPU and moved to ``b``'s device and dtype, the ranks capped at the
    largest the shape admits; one of the two is needed.  A sweep goes left to right and back.  Every local system is solved by
    at most ``local_iters`` conjugate-gradient steps from the current core, down to ``||r|| <= (tol / 10) ||f||``; the largest
    relative residual the sites had BEFORE their solves is read back once per sweep, and the sweeps stop when it is ``<= tol``
    or after ``nswp`` of them.  ``tol=None``: ``sqrt(eps)`` of the dtype (3.45e-4 in fp32, 1.49e-8 in fp64).  ``verbose``
    prints one line per sweep.  ``b == 0`` returns the rank-1 zero train.  Tucker factors of ``b`` and ``x0`` are contracted in.

    ``return_info=True`` returns ``(x, info)`` with ``sweeps``, ``converged``, ``local_residuals`` (one float per sweep) and
    ``residual``, ``||tt_apply(M, x) - b|| / ||b||``, computed once at the end: the difference train is orthogonalised and the
    norm of its last core taken, so nothing cancels and its rounding floor is a few ``N eps (||M x|| + ||b||) / ||b||`` (the
    ``sqrt(eps)`` floor of ``tn.relative_error`` between two trains does not apply).

    The call runs under ``torch.no_grad()`` and returns detached cores; on the device an operand that requires grad raises
    ``NotImplementedError`` under grad mode."""
    who = "tt_solve"
    G, trains = _check_system(who, tt_matrix, b, x0)
    if x0 is None and ranks_tt is None:
        raise ValueError("{}: give x0 or ranks_tt (the ranks of the solution are fixed)".format(who))
    _check_controls(who, nswp, local_iters, tol)
    _check_devices(who, G, trains)
    with torch.no_grad():
        return _solve(tt_matrix, b, bool(transpose), x0, ranks_tt, int(nswp), tol, int(local_iters), verbose, return_info)


def _check_system(who: str, tt_matrix, b, x0):
    """The operand checks of the TT solvers (tt_solve, tt_amen_solve), in their order: the matrix, then ``b`` and ``x0`` (class,
    batch, CP cores, modes, boundary ranks), then square modes of one size.  Returns the matrix cores and the named trains."""
    G = _matrix_cores(who, "the first argument", tt_matrix)
    N = len(G)
    trains = [("b", b)] + ([("x0", x0)] if x0 is not None else [])
    for name, t in trains:
        if not isinstance(t, Tensor):
            raise ValueError("{}: {} must be a tntorch_amd.Tensor, got {}".format(who, name, type(t).__name__))
        if t.batch:
            raise ValueError("{}: batched tensors are not supported ({})".format(who, name))
        if any(c.dim() == 2 for c in t.cores):
            _not_in_scope("{} with CP cores".format(who))
        if t.dim() != N:
            raise ValueError("{}: the matrix has {} modes, {} has {}".format(who, N, name, t.dim()))
        if t.cores[0].shape[0] != 1 or t.cores[-1].shape[-1] != 1:
            raise ValueError("{}: the boundary ranks of {} must be 1, got {} and {}".format(
                who, name, t.cores[0].shape[0], t.cores[-1].shape[-1]))
    for k, g in enumerate(G):
        if int(g.shape[1]) != int(g.shape[2]):
            raise ValueError("{}: mode {} of the matrix is not square: {} x {}".format(who, k, int(g.shape[1]), int(g.shape[2])))
        for name, t in trains:
            if int(t.shape[k]) != int(g.shape[1]):
                raise ValueError("{}: mode {} of {} has size {}, the matrix's {}".format(who, k, name, int(t.shape[k]), int(g.shape[1])))
    return G, trains


def _check_controls(who: str, nswp, local_iters, tol) -> None:
    if int(nswp) < 1 or int(local_iters) < 1:
        raise ValueError("{}: nswp and local_iters must be at least 1, got {} and {}".format(who, nswp, local_iters))
    if tol is not None and not float(tol) > 0:
        raise ValueError("{}: tol must be positive, got {}".format(who, tol))


def _check_devices(who: str, G, trains) -> None:
    """One device and dtype for the matrix and the trains; on the device under grad mode an operand that requires grad is refused."""
    tensors = []
    for _, t in trains:
        tensors += list(t.cores) + [U for U in t.Us if U is not None]
    if _check_operands(who, G, tensors) and torch.is_grad_enabled():
        _refuse_device_grad(who)


def _solve(tt_matrix, b, transpose, x0, ranks_tt, nswp, tol, local_iters, verbose, return_info):
    detach = lambda t: Tensor([c.detach() for c in t.cores], Us=[None if U is None else U.detach() for U in t.Us])  # noqa: E731
    b = detach(b)
    b4 = b._absorbed4()
    bc = [c[0] for c in b4]                                   # [c, n, c']
    dtype, device = bc[0].dtype, bc[0].device
    N, shape = len(bc), [int(c.shape[1]) for c in bc]
    ops = ops_for(bc[0])
    # the operator as cores A_k [a, i, j, a'] with (A x)[i] = sum_j A[i, j] x[j]: vec(x) @ M reads the transposed views
    M = type(tt_matrix)([g.detach() for g in tt_matrix.cores], None, tt_matrix.input_dims.tolist(), tt_matrix.output_dims.tolist())
    A = (M if transpose else tt_transpose(M)).cores
    tol = math.sqrt(torch.finfo(dtype).eps) if tol is None else float(tol)
    info = {"sweeps": 0, "converged": True, "local_residuals": [], "residual": 0.0}

    bnorm = _read("setup", ops.dot(b4, b4))[0]
    if not bnorm > 0:
        x = Tensor([torch.zeros((1, n, 1), dtype=dtype, device=device) for n in shape])
        return (x, info) if return_info else x
    bnorm = math.sqrt(bnorm)

    if x0 is not None:
        xs = [c.clone() for c in detach(x0)._absorbed4()]     # [1, r, n, s]
    else:
        from .create import rand

        want = list(ranks_tt) if hasattr(ranks_tt, "__len__") else [ranks_tt] * (N - 1)
        if len(want) != N - 1:
            raise ValueError("tt_solve: ranks_tt needs {} entries, got {}".format(N - 1, len(want)))
        ranks = [max(1, min(int(r), cap)) for r, cap in zip(want, _max_ranks(shape))]
        start = rand(shape, ranks_tt=ranks) if N > 1 else rand(shape, ranks_tt=[])
        xs = [c.to(device=device, dtype=dtype)[None] for c in start.cores]

    one = lambda *s: torch.ones(s, dtype=dtype, device=device)  # noqa: E731
    for mu in range(N - 1, 0, -1):
        ops.right_orthogonalize(xs, mu)
    Phi: List[Optional[torch.Tensor]] = [None] * N
    Psi: List[Optional[torch.Tensor]] = [None] * N
    phi: List[Optional[torch.Tensor]] = [None] * N
    psi: List[Optional[torch.Tensor]] = [None] * N
    Phi[0], phi[0], Psi[N - 1], psi[N - 1] = one(1, 1, 1), one(1, 1), one(1, 1, 1), one(1, 1)

    def move(side: str, k: int):
        xk = xs[k][0]
        if side == "left":
            Phi[k + 1] = ops.env_update("left", Phi[k], A[k], xk, xk)
            phi[k + 1] = _rhs_update(ops, "left", phi[k], bc[k], xk)
        else:
            Psi[k - 1] = ops.env_update("right", Psi[k], A[k], xk, xk)
            psi[k - 1] = _rhs_update(ops, "right", psi[k], bc[k], xk)

    for k in range(N - 1, 0, -1):
        move("right", k)

    stat = torch.zeros(2, dtype=dtype, device=device)         # [largest first residual of the sweep, steps with p^T B p <= 0]

    def solve(k: int):
        f = _rhs_local(ops, phi[k], bc[k], psi[k])
        xs[k] = _cg(ops, Phi[k], A[k], Psi[k], f, xs[k][0], tol / 10.0, local_iters, stat)[None]

    info["converged"] = False
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
        worst, bad = _read("sweep", stat)
        if bad > 0 or not math.isfinite(worst):
            raise ValueError("tt_solve: the matrix is not positive definite (a local CG step met p^T B p <= 0 in sweep {})".format(
                sweep + 1))
        info["sweeps"] = sweep + 1
        info["local_residuals"].append(worst)
        if verbose:
            print("tt_solve: sweep {:3d}  largest local residual {:.3e}".format(sweep + 1, worst))
        if worst <= tol:
            info["converged"] = True
            break

    x = Tensor([c[0] for c in xs])
    if not return_info:
        return x
    diff = tt_apply(M, x, transpose=transpose) - b
    info["residual"] = _read("residual", _tt_norm(ops, diff._absorbed4()))[0] / bnorm
    return x, info

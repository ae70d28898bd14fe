"""``tt_amen_solve``: the train ``x`` with ``tt_apply(M, x) ~ b`` for a symmetric positive definite ``TTMatrix`` ``M`` and a
``Tensor`` ``b``, with ranks that adapt while the sweeps run: AMEn in the ALS(t+z) form of Dolgov and Savostyanov (SIAM J. Sci.
Comput. 36, 2014).  ``tt_solve`` (ttsolve.py) is the same one-site ALS at ranks the caller fixes.

A sweep goes left to right.  At site ``k`` the local system ``B_k v = f_k`` of ``tt_solve`` is solved by conjugate gradients
(``ops.cg_solve``: on the device three launches of ttr_cg.hip between two matvecs, on the CPU ``ttsolve._cg`` itself), and the
left unfolding of ``v`` is truncated to ``U W`` at ``eps / sqrt(N)``.  Then the residual ``b - A x`` at the truncated core is
projected twice, with the interfaces of a second, auxiliary train ``z`` of ranks ``kickrank`` on the right:

    z_k = rhs(phi_zb, b_k, psi_zb) - B(Phi_zx, A_k, Psi_zx) U W        [rho_{k-1}, n_k, rho_k]   the next core of z (its Q)
    e_k = rhs(phi_xb, b_k, psi_zb) - B(Phi_xx, A_k, Psi_zx) U W        [r_{k-1},   n_k, rho_k]   the enrichment of x

``[U, e_k]`` is the new core and ``W x_{k+1}`` with rows of zeros appended the next one: the tensor is unchanged, but the basis of
the next local problem holds directions of the residual, which is what lets a rank grow.  Eight interface stacks are carried,
(x, A, x), (x, b), (z, A, x) and (z, b) from the left and from the right; they are launches of ``env_update`` and
``_rhs_update`` with a bra that differs from the ket.  The return leg solves nothing: it right-orthogonalises ``x`` and ``z``
and rebuilds the right stacks.  After the last sweep the train is rounded once, which drops the directions no solve used.

Not here: solves on the return leg (two-directional AMEn), a residual-based stopping rule instead of the local one,
nonsymmetric local solvers, a preconditioner, a kernel for the initialisation of a local CG, batched operands and the device
backward.
"""

from __future__ import annotations

import math
from typing import List, Optional

import torch

from ._dispatch import ops_for
from .tensor import Tensor
from .ttalgebra import tt_apply, tt_transpose
from .ttsolve import _check_controls, _check_devices, _check_system, _max_ranks, _rhs_local, _rhs_update, _tt_norm

__all__ = ["tt_amen_solve"]

# how often the driver has read device scalars back, by kind ("sweep": the stopping value and the flag, once per sweep; "setup":
# ||b||; "residual": the final residual of return_info; "round": calls of the final round_tt, which reads the ranks it decides).
# The truncation of a solved core decides a rank and reads it in ``ops.truncated_svd``; that is not counted here.
READBACKS = {"sweep": 0, "setup": 0, "residual": 0, "round": 0}


def _read(kind: str, t: torch.Tensor) -> List[float]:
    READBACKS[kind] += 1
    return [float(v) for v in t.detach().cpu().reshape(-1).tolist()]


def tt_amen_solve(tt_matrix, b, transpose: bool = False, x0: Optional[Tensor] = None, kickrank: int = 2, rmax: Optional[int] = None,
                  nswp: int = 20, tol=None, eps=None, local_iters: int = 50, seed: int = 0, verbose: bool = False,
                  return_info: bool = False):
    """The train ``x`` with ``tn.tt_apply(tt_matrix, x, transpose=transpose)`` approximately ``b``, at ranks found while solving:
    by default the solution of ``vec(x) @ M = vec(b)``, with ``transpose=True`` of ``M @ vec(x) = vec(b)`` (``tt_solve``'s
    conventions).  The matrix must be square in every mode and symmetric positive definite.  Symmetry is NOT checked; a loss of
    positive definiteness is detected -- a local CG step with ``p^T B p <= 0`` -- and raises ``ValueError`` at the end of the sweep.

    AMEn: left-to-right sweeps of one-site solves; each solved core is truncated at ``eps / sqrt(N)`` (``eps=None``:
    ``tol / 10``) and enriched by up to ``kickrank`` directions of the projected residual, every rank capped by ``rmax`` and by
    the largest the shape admits.  ``kickrank=0`` is one-site ALS with truncation: ranks can fall but not grow.  The start is
    ``x0`` if it is given (never written; its Tucker factors are contracted in), else a rank-1 train drawn on the CPU from
    ``torch.Generator().manual_seed(seed)`` and moved to ``b``'s device and dtype; the auxiliary train comes from the same
    generator, so a call is deterministic given its arguments.  Every local system is solved by at most ``local_iters``
    conjugate-gradient steps from the current core, down to ``||r|| <= (tol / 10) ||f||``; the largest relative residual the
    sites had BEFORE their solves is read back once per sweep, and the sweeps stop when it is ``<= tol`` or after ``nswp`` of
    them.  ``tol=None``: ``sqrt(eps)`` of the dtype.  After the last sweep the train is rounded once with
    ``round_tt(eps=eps, rmax=rmax)``.  ``b == 0`` returns the rank-1 zero train.  ``verbose`` prints one line per sweep.

    ``return_info=True`` returns ``(x, info)`` with ``sweeps``, ``converged``, ``local_residuals`` (one float per sweep), ``ranks``
    (the TT ranks after each sweep, before the final rounding) and ``residual``, ``||tt_apply(M, x) - b|| / ||b||`` of the
    returned train, computed as in ``tt_solve``.

    Raises ``ValueError`` for what ``tt_solve`` refuses and for ``kickrank < 0``, ``rmax < 1`` and ``eps <= 0``,
    ``NotImplementedError`` for CP cores.  The call runs under ``torch.no_grad()`` and returns detached cores; on the device an
    operand that requires grad raises ``NotImplementedError`` under grad mode."""
    who = "tt_amen_solve"
    G, trains = _check_system(who, tt_matrix, b, x0)
    _check_controls(who, nswp, local_iters, tol)
    if int(kickrank) < 0:
        raise ValueError("{}: kickrank must not be negative, got {}".format(who, kickrank))
    if rmax is not None and int(rmax) < 1:
        raise ValueError("{}: rmax must be at least 1, got {}".format(who, rmax))
    if eps is not None and not float(eps) > 0:
        raise ValueError("{}: eps must be positive, got {}".format(who, eps))
    _check_devices(who, G, trains)
    with torch.no_grad():
        return _amen(tt_matrix, b, bool(transpose), x0, int(kickrank), None if rmax is None else int(rmax), int(nswp), tol, eps,
                     int(local_iters), int(seed), verbose, return_info)


def _amen(tt_matrix, b, transpose, x0, kickrank, rmax, nswp, tol, eps, local_iters, seed, verbose, return_info):
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
    eps = tol / 10.0 if eps is None else float(eps)
    info = {"sweeps": 0, "converged": True, "local_residuals": [], "ranks": [], "residual": 0.0}

    bnorm = _read("setup", ops.dot(b4, b4))[0]
    if not bnorm > 0:
        x = Tensor([torch.zeros((1, n, 1), dtype=dtype, device=device) for n in shape])
        return (x, info) if return_info else x
    bnorm = math.sqrt(bnorm)

    caps = _max_ranks(shape)
    cap = [c if rmax is None else min(c, rmax) for c in caps]  # the largest rank bond k may take
    gen = torch.Generator().manual_seed(seed)
    draw = lambda r, n, s: torch.randn((1, r, n, s), generator=gen, dtype=torch.float64).to(device=device, dtype=dtype)  # noqa: E731
    if x0 is not None:
        xs = [c.clone() for c in detach(x0)._absorbed4()]     # [1, r, n, s]
    else:
        xs = [draw(1, n, 1) for n in shape]
    rho = [1] + [min(kickrank, c) for c in caps] + [1]        # the ranks of z, boundary ones included
    zs = [draw(rho[k], shape[k], rho[k + 1]) for k in range(N)] if kickrank > 0 else None
    for mu in range(N - 1, 0, -1):
        ops.right_orthogonalize(xs, mu)
        if zs is not None:
            ops.right_orthogonalize(zs, mu)

    one = lambda *s: torch.ones(s, dtype=dtype, device=device)  # noqa: E731
    left = lambda first: [first] + [None] * (N - 1)           # noqa: E731
    right = lambda last: [None] * (N - 1) + [last]            # noqa: E731
    # the interfaces LEFT of site k (Phi, phi) and RIGHT of it (Psi, psi), of (x, A, x), (x, b), (z, A, x) and (z, b)
    Phi_xx, Psi_xx, phi_xb, psi_xb = left(one(1, 1, 1)), right(one(1, 1, 1)), left(one(1, 1)), right(one(1, 1))
    Phi_zx, Psi_zx, phi_zb, psi_zb = left(one(1, 1, 1)), right(one(1, 1, 1)), left(one(1, 1)), right(one(1, 1))

    def move_right(k: int):
        xk = xs[k][0]
        Psi_xx[k - 1] = ops.env_update("right", Psi_xx[k], A[k], xk, xk)
        psi_xb[k - 1] = _rhs_update(ops, "right", psi_xb[k], bc[k], xk)
        if zs is not None:
            zk = zs[k][0]
            Psi_zx[k - 1] = ops.env_update("right", Psi_zx[k], A[k], zk, xk)
            psi_zb[k - 1] = _rhs_update(ops, "right", psi_zb[k], bc[k], zk)

    def move_left(k: int):
        xk = xs[k][0]
        Phi_xx[k + 1] = ops.env_update("left", Phi_xx[k], A[k], xk, xk)
        phi_xb[k + 1] = _rhs_update(ops, "left", phi_xb[k], bc[k], xk)
        if zs is not None:
            zk = zs[k][0]
            Phi_zx[k + 1] = ops.env_update("left", Phi_zx[k], A[k], zk, xk)
            phi_zb[k + 1] = _rhs_update(ops, "left", phi_zb[k], bc[k], zk)

    for k in range(N - 1, 0, -1):
        move_right(k)

    stat = torch.zeros(2, dtype=dtype, device=device)         # [largest first residual of the sweep, steps with p^T B p <= 0]

    def site(k: int):
        f = _rhs_local(ops, phi_xb[k], bc[k], psi_xb[k])
        v = ops.cg_solve(Phi_xx[k], A[k], Psi_xx[k], f, xs[k][0], tol / 10.0, local_iters, stat)
        if k == N - 1:
            xs[k] = v[None]
            return
        r, n, s = v.shape
        U, W = ops.truncated_svd(v.reshape(1, r * n, s), None, eps / math.sqrt(N), rmax, True, "svd", False)
        U, W = U[0].to(dtype), W[0].to(dtype)                 # [r n, r'], [r', s]
        rk = U.shape[1]
        nxt = xs[k + 1][0]
        nxt = ops.gemm2d(W, nxt.reshape(s, -1))               # [r', n' s']
        add = 0
        if zs is not None:
            vt = ops.gemm2d(U, W).reshape(r, n, s)
            zk = _rhs_local(ops, phi_zb[k], bc[k], psi_zb[k]) - ops.local_matvec(Phi_zx[k], A[k], Psi_zx[k], vt)
            add = max(0, min(rho[k + 1], min(r * n, cap[k]) - rk))
            if add > 0:
                ek = _rhs_local(ops, phi_xb[k], bc[k], psi_zb[k]) - ops.local_matvec(Phi_xx[k], A[k], Psi_zx[k], vt)
                U = torch.cat([U, ek.reshape(r * n, rho[k + 1])[:, :add]], dim=1)
                nxt = torch.cat([nxt, nxt.new_zeros((add, nxt.shape[1]))], dim=0)
            Q, _ = ops.qr(zk.reshape(1, rho[k] * n, rho[k + 1]))
            zs[k] = Q.reshape(1, rho[k], n, rho[k + 1])
        xs[k] = U.reshape(1, r, n, rk + add)
        xs[k + 1] = nxt.reshape(1, rk + add, shape[k + 1], -1)
        ops.left_orthogonalize(xs, k)
        move_left(k)

    info["converged"] = False
    for sweep in range(nswp):
        stat.zero_()
        for k in range(N):
            site(k)
        worst, bad = _read("sweep", stat)
        if bad > 0 or not math.isfinite(worst):
            raise ValueError("tt_amen_solve: the matrix is not positive definite (a local CG step met p^T B p <= 0 in sweep {})".format(
                sweep + 1))
        info["sweeps"] = sweep + 1
        info["local_residuals"].append(worst)
        info["ranks"].append([int(c.shape[3]) for c in xs[:-1]])
        if verbose:
            print("tt_amen_solve: sweep {:3d}  largest local residual {:.3e}  ranks {}".format(sweep + 1, worst, info["ranks"][-1]))
        if worst <= tol:
            info["converged"] = True
            break
        if sweep + 1 < nswp:                                  # the return leg: no solves
            for k in range(N - 1, 0, -1):
                ops.right_orthogonalize(xs, k)
                if zs is not None:
                    ops.right_orthogonalize(zs, k)
                move_right(k)

    if N > 1:
        READBACKS["round"] += 1
        xs = ops.round_tt(xs, eps, [rmax] * (N - 1), "svd", False, None)
    x = Tensor([c[0] for c in xs])
    if not return_info:
        return x
    diff = tt_apply(M, x, transpose=transpose) - b
    info["residual"] = _read("residual", _tt_norm(ops, diff._absorbed4()))[0] / bnorm
    return x, info

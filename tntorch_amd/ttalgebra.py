"""``tt_apply``, ``tt_matmul``, ``tt_transpose``: products of a ``TTMatrix`` with a ``Tensor`` and with another ``TTMatrix`` that
stay in TT format.  ``tt_multiply`` and ``tt_lookup`` meet a TT-matrix with DENSE data; applying one to a
train through them means ``t.torch()``, ``prod(input_dims)`` numbers, which defeats both formats exactly where a TT-matrix is
worth having.  Here nothing dense is formed: the result's cores are built mode by mode, its ranks are the products of the
operands' ranks, and ``round_tt`` brings them back down -- the building block of time stepping ``u <- round(u + dt A u)``, power
iteration, composed operators ``A B`` and a TT layer fed with a compressed input.

Everything rests on one identity.  For ``A [R1, P, J, R2]`` and ``B [S1, J, Q, S2]``

    compose(A, B)[r S1 + a, p, q, s S2 + b] = sum_j A[r, p, j, s] B[a, j, q, b]            -> [R1 S1, P, Q, R2 S2]

(the rank layout of ``core_kron``: the first operand's rank major).  With ``G_k [r, I_k, O_k, s]`` the cores of a TT-matrix
``M``, ``T_k [a, n, b]`` those of a train and ``H_k`` those of a second TT-matrix, core ``k`` of

    vec(t) @ M     is   compose(T_k[:, None], G_k)[:, 0]          (P = 1, J = I_k)
    M @ vec(u)     is   compose(G_k, U_k[:, :, None])[:, :, 0]    (Q = 1, J = O_k)
    A @ B          is   compose(G_k, H_k)                         (J = O_k(A) = I_k(B))

One ``core_compose`` per mode: on device tensors one launch of ``ttr_core_compose`` (a GEMM over ``j`` on the matrix cores whose
output is written once, in memory order), on the CPU one einsum, which autograd differentiates.

Not here: a fused apply-and-round (zip-up or variational) that never stores the cores of rank ``r s``, the backward on the device
(device operands that require grad are refused under grad mode, not detached silently), batched operands and CP-matrices,
``TTMatrix`` arithmetic sugar (``@``, ``+``) and a strided-operand path in the kernel (views are copied first).
"""

from __future__ import annotations

from typing import List

import torch

from ._dispatch import ops_for
from .matrix import TTMatrix
from .tensor import Tensor, _not_in_scope

__all__ = ["tt_apply", "tt_matmul", "tt_transpose"]


def _matrix_cores(who: str, what: str, m) -> List[torch.Tensor]:
    if not isinstance(m, TTMatrix):
        raise ValueError("{}: {} must be a TTMatrix, got {}".format(who, what, type(m).__name__))
    cores = list(m.cores)
    if any(c.dim() != 4 for c in cores):
        raise ValueError("{}: batched matrices ({}-D cores) are not supported".format(who, cores[0].dim()))
    if cores[0].shape[0] != 1 or cores[-1].shape[-1] != 1:
        raise ValueError("{}: the boundary ranks must be 1, got {} and {}".format(who, cores[0].shape[0], cores[-1].shape[-1]))
    return cores


def _check_operands(who: str, first: List[torch.Tensor], second: List[torch.Tensor]):
    """dtype, device and grad checks of the two operands' tensors (cores, and factors where a train has them); returns the pair
    with everything detached where that is the only way to run (device tensors that require grad while grad mode is off)."""
    dtype, device = first[0].dtype, first[0].device
    if dtype not in (torch.float32, torch.float64):
        raise ValueError("{}: float32 or float64 operands are needed, got {}".format(who, dtype))
    if any(x.dtype != dtype for x in first + second):
        raise ValueError("{}: the operands must have the same dtype".format(who))
    if any(x.device != device for x in first + second):
        raise ValueError("{}: the operands must be on the same device".format(who))
    return device.type != "cpu" and any(x.requires_grad for x in first + second)


def _refuse_device_grad(who: str):
    raise NotImplementedError("tntorch_amd: {} is not differentiable on the device (the products that stay in TT format have no "
                              "backward kernels); detach the cores or use CPU tensors".format(who))


def _separable(cores) -> bool:
    return all(c.shape[0] == 1 and c.shape[-1] == 1 for c in cores)


def tt_transpose(A: TTMatrix) -> TTMatrix:
    """The transposed TT-matrix: every core ``[r, i, o, s]`` seen as ``[r, o, i, s]`` (``permute(0, 2, 1, 3)`` views of the same
    storage) and the dims swapped; nothing is copied."""
    if not isinstance(A, TTMatrix):
        raise ValueError("tt_transpose: the argument must be a TTMatrix, got {}".format(type(A).__name__))
    if any(c.dim() != 4 for c in A.cores):
        raise ValueError("tt_transpose: batched matrices ({}-D cores) are not supported".format(A.cores[0].dim()))
    return TTMatrix([c.permute(0, 2, 1, 3) for c in A.cores], None, A.output_dims.tolist(), A.input_dims.tolist())


def tt_apply(tt_matrix: TTMatrix, t: Tensor, transpose: bool = False, eps=None, rmax=None, algorithm: str = "svd") -> Tensor:
    """The train of ``vec(t) @ M`` (``tt_multiply``'s convention: ``t.shape == input_dims``, the result has shape
    ``output_dims`` and ``tt_apply(M, t).torch().reshape(-1)`` is ``tt_multiply(M, t.torch().reshape(1, -1))[0]``), or with
    ``transpose=True`` of ``M @ vec(t)`` (``t.shape == output_dims``, the result has shape ``input_dims``), without anything
    dense: one ``core_compose`` per mode.  The TT ranks are the products of the operands' ranks, the first factor of the product
    major (the train's for the default, the matrix's for ``transpose=True``).  Tucker factors of ``t`` are contracted in first.

    ``eps is None and rmax is None``: the exact, unrounded train.  Otherwise one ``round_tt(eps=eps or 0, rmax=rmax,
    algorithm=algorithm)``; when every rank of one operand is 1 the ranks do not grow and, for ``rmax=None``, nothing is rounded.
    Neither operand is modified; the result is on the operands' device in their dtype.  On the CPU the chain is plain torch and
    differentiable; on the device an operand that requires grad raises ``NotImplementedError`` under grad mode."""
    who = "tt_apply"
    G = _matrix_cores(who, "the first argument", tt_matrix)
    if not isinstance(t, Tensor):
        raise ValueError("{}: t must be a tntorch_amd.Tensor, got {}".format(who, type(t).__name__))
    if t.batch:
        raise ValueError("{}: batched tensors are not supported".format(who))
    if any(c.dim() == 2 for c in t.cores):
        _not_in_scope("tt_apply of CP cores")
    if t.dim() != len(G):
        raise ValueError("{}: the matrix has {} modes, the tensor {}".format(who, len(G), t.dim()))
    side = 2 if transpose else 1   # the matrix axis the tensor's modes meet
    for k, (g, n) in enumerate(zip(G, t.shape)):
        if int(g.shape[side]) != int(n):
            raise ValueError("{}: mode {} of the tensor has size {}, the matrix's {} mode {}".format(
                who, k, int(n), "output" if transpose else "input", int(g.shape[side])))
    factors = [U for U in t.Us if U is not None]
    if _check_operands(who, G, list(t.cores) + factors):
        if torch.is_grad_enabled():
            _refuse_device_grad(who)
        G = [g.detach() for g in G]
        t = Tensor([c.detach() for c in t.cores], Us=[None if U is None else U.detach() for U in t.Us])
    T = [c[0] for c in t._absorbed4()]   # [a, n, b]
    ops = ops_for(G[0])
    if transpose:
        cores = [ops.core_compose(g, u[:, :, None, :])[:, :, 0] for g, u in zip(G, T)]
    else:
        cores = [ops.core_compose(x[:, None], g)[:, 0] for x, g in zip(T, G)]
    out = Tensor(cores)
    if (eps is None and rmax is None) or (rmax is None and (_separable(G) or _separable(T))):
        return out
    out.round_tt(eps=eps or 0, rmax=rmax, algorithm=algorithm)
    return out


def tt_matmul(A: TTMatrix, B: TTMatrix, eps=None, rmax=None, algorithm: str = "svd") -> TTMatrix:
    """The TT-matrix of ``A.torch() @ B.torch()``: core ``k`` is ``compose(A_k, B_k)``, one ``core_compose`` per mode.  It needs
    ``A.output_dims == B.input_dims``; the result has ``A.input_dims`` and ``B.output_dims``, and ranks that are the products,
    ``A``'s major.  Rounding as ``tt_apply`` does it, on the flattened train (``TTMatrix.flatten()``), whose cores are reshaped
    back.  Neither operand is modified."""
    who = "tt_matmul"
    GA = _matrix_cores(who, "the first argument", A)
    GB = _matrix_cores(who, "the second argument", B)
    if len(GA) != len(GB):
        raise ValueError("{}: the matrices have {} and {} modes".format(who, len(GA), len(GB)))
    for k, (a, b) in enumerate(zip(GA, GB)):
        if int(a.shape[2]) != int(b.shape[1]):
            raise ValueError("{}: mode {}: the first matrix's output mode has size {}, the second's input mode {}".format(
                who, k, int(a.shape[2]), int(b.shape[1])))
    if _check_operands(who, GA, GB):
        if torch.is_grad_enabled():
            _refuse_device_grad(who)
        GA, GB = [g.detach() for g in GA], [g.detach() for g in GB]
    ops = ops_for(GA[0])
    cores = [ops.core_compose(a, b) for a, b in zip(GA, GB)]
    idims, odims = [int(c.shape[1]) for c in cores], [int(c.shape[2]) for c in cores]
    out = TTMatrix(cores, None, idims, odims)
    if (eps is None and rmax is None) or (rmax is None and (_separable(GA) or _separable(GB))):
        return out
    flat = out.flatten()
    flat.round_tt(eps=eps or 0, rmax=rmax, algorithm=algorithm)
    return TTMatrix([c.reshape(c.shape[0], idims[k], odims[k], c.shape[-1]) for k, c in enumerate(flat.cores)], None, idims, odims)

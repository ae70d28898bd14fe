"""``tt_lookup``: a batch of rows of a ``TTMatrix``, ``M[rows, :]``, without the dense matrix -- the embedding table kept as a
TT-matrix (TT-Rec, TT embeddings), next to the TT linear layer ``tt_multiply``.

Row ``j`` splits row-major into the digits ``(i_1 .. i_d)`` over ``input_dims``, ``i_1`` most significant (the order of
``TTMatrix.__init__``'s ``M.reshape(idims + odims)``), and

    y[p, (o_1 .. o_d)] = G_1[0, i_1, o_1, :] G_2[:, i_2, o_2, :] ... G_d[:, i_d, o_d, 0]

runs as a chain with the state ``Z_k [P, D_k, r_k]``, ``D_k = O_1 .. O_k``: ``Z_k[p, (dd, o), s] = sum_r Z_{k-1}[p, dd, r]
G_k[r, i_k(p), o, s]``.  The row-major output of a step is the next step's input as it lies.  On the device a step is one
launch of ``ttr_ttm_lookup_step``: the samples are grouped by ``i_k`` so that those of a group share their slice of the core,
and each group is a GEMM on the matrix cores.  On the CPU the chain is plain torch, and therefore differentiable in the cores.
``tt_lookup`` itself refuses device cores that require grad (it raises instead of cutting the graph): the trainable lookup is
``embedding.py``'s ``tt_embedding`` / ``tt_embedding_bag``.  Not here: a CP-matrix lookup, the deduplication of
repeated rows and a kernel for the whole chain.
"""

from __future__ import annotations

import torch

from ._dispatch import ops_for
from .matrix import TTMatrix

__all__ = ["tt_lookup"]


def lookup_operands(who: str, tt_matrix, rows):
    """The checks ``tt_lookup`` and the calls of ``embedding.py`` share: ``(cores, rows, cols)`` with ``rows`` an int32 / int64
    tensor on the cores' device (a list / tuple / numpy array of ints is placed there) and ``cols`` the number of columns;
    ``ValueError`` (``who`` names the caller) for anything else."""
    if not isinstance(tt_matrix, TTMatrix):
        raise ValueError("{}: the first argument must be a TTMatrix, got {}".format(who, type(tt_matrix).__name__))
    cores = tt_matrix.cores
    if any(c.dim() != 4 for c in cores):
        raise ValueError("{}: batched matrices ({}-D cores) are not supported".format(who, cores[0].dim()))
    if cores[0].shape[0] != 1 or cores[-1].shape[-1] != 1:
        raise ValueError("{}: the boundary ranks must be 1, got {} and {}".format(who, cores[0].shape[0], cores[-1].shape[-1]))
    dtype, device = cores[0].dtype, cores[0].device
    if dtype not in (torch.float32, torch.float64):
        raise ValueError("{}: float32 or float64 cores are needed, got {}".format(who, dtype))
    if any(c.dtype != dtype for c in cores):
        raise ValueError("{}: the cores must have the same dtype".format(who))
    if any(c.device != device for c in cores):
        raise ValueError("{}: the cores must be on the same device".format(who))
    if not isinstance(rows, torch.Tensor):
        rows = torch.as_tensor(rows)
        if rows.numel() == 0 and rows.is_floating_point():   # (an empty list has no dtype of its own)
            rows = rows.to(torch.int64)
        if rows.dtype in (torch.int32, torch.int64):
            rows = rows.to(device)
    if rows.dtype not in (torch.int32, torch.int64):
        raise ValueError("{}: the rows must be int32 or int64 indices, got {}".format(who, rows.dtype))
    if rows.device != device:
        raise ValueError("{}: the matrix and the rows must be on the same device".format(who))
    cols = 1
    for c in cores:
        cols *= int(c.shape[2])
    return cores, rows, cols


def tt_lookup(tt_matrix: TTMatrix, rows) -> torch.Tensor:
    """``tt_matrix.torch()[rows]`` -> ``rows.shape + (cols,)`` on the cores' device in their dtype, without forming the matrix.
    ``rows``: an integer tensor of any shape (int32 / int64, on the cores' device), or a list / tuple / numpy array of ints
    (placed there); negative entries wrap as in torch, a row outside ``[-rows, rows)`` raises ``IndexError``.  On the device:
    ``d - 1`` launches of ``ttr_ttm_lookup_step`` (``d = 1``: an ``index_select``) and one readback of the out-of-range word.
    Neither operand is modified.  Under grad mode a device core that requires grad raises ``NotImplementedError``:
    ``tn.tt_embedding`` is the same lookup, differentiable in the cores on every device."""
    cores, rows, cols = lookup_operands("tt_lookup", tt_matrix, rows)
    dtype, device = cores[0].dtype, cores[0].device
    shape = tuple(rows.shape) + (cols,)
    if rows.numel() == 0:
        return torch.zeros(shape, dtype=dtype, device=device)
    if device.type != "cpu" and torch.is_grad_enabled() and any(c.requires_grad for c in cores):
        # (ops_for refuses a FIRST core that requires grad; the others would come back detached, silently)
        raise NotImplementedError("tntorch_amd: tt_lookup is not differentiable on the device; detach the cores or use CPU tensors")
    ops = ops_for(cores[0].detach() if device.type != "cpu" else cores[0])
    return ops.tt_lookup_chain(cores, rows.reshape(-1)).reshape(shape)

"""``tt_embedding`` and ``tt_embedding_bag``: the embedding table kept as a ``TTMatrix`` (TT-Rec, TT embeddings), TRAINABLE on
every device.  Named after ``torch.nn.functional.embedding`` / ``embedding_bag``; ``lookup.py``'s ``tt_lookup``
is the same gather without a backward on the device.

The forward is ``tt_lookup``'s chain (``lookup.py``): the state ``Z_k [P, D_k, r_k]`` grows by one core per step.  Backwards, with
``dY_k`` the gradient of ``Z_k`` read as ``[P, D_{k-1}, O_k, r_k]``,

    dG_k[r, i, o, s]   = sum_{p: i_k(p) = i} sum_dd Z_{k-1}[p, dd, r] dY_k[p, dd, o, s]        ttr_ttm_lookup_grad_core
    dZ_{k-1}[p, dd, r] = sum_{o, s} dY_k[p, dd, o, s] G_k[r, i_k(p), o, s]                     ttr_ttm_lookup_grad_input
    dG_1[0, i, :, :]   = sum_{p: i_1(p) = i} dZ_1[p]                                           ttr_segment_sum

and a bag is the segmented sum of its rows (``ttr_segment_sum`` again).  On the device this is one ``torch.autograd.Function``
(``autodiff.tt_rows``) that keeps the states the core gradients need -- the memory cost of training -- and synchronises once, in
the forward.  On the CPU both calls are plain torch, and autograd does the rest.

Not here: the gradient of ``per_sample_weights``, ``mode="max"``, ``padding_idx``, ``include_last_offset``, an ``nn.Module``
wrapper, pooling fused into the last step, the deduplication of repeated rows, double backward and a CP-matrix table.
"""

from __future__ import annotations

from typing import Optional

import torch

from . import _hostops, autodiff
from ._dispatch import ops_for
from .lookup import lookup_operands
from .matrix import TTMatrix

__all__ = ["tt_embedding", "tt_embedding_bag"]


def _wants_grad(cores) -> bool:
    return torch.is_grad_enabled() and any(c.requires_grad for c in cores)


def tt_embedding(ttm: TTMatrix, rows) -> torch.Tensor:
    """``ttm.torch()[rows]`` -> ``rows.shape + (cols,)``, differentiable in the cores on every device.  ``rows`` as for
    ``tn.tt_lookup``: an int32 / int64 tensor of any shape on the cores' device, or a list / tuple / numpy array of ints;
    negative rows wrap, a row outside ``[-rows, rows)`` raises ``IndexError``.  With no core that requires grad, or under
    ``torch.no_grad()``, it runs ``tt_lookup``'s launches and returns its bits; otherwise the device keeps the states the core
    gradients need (``autodiff.tt_rows``)."""
    cores, rows, cols = lookup_operands("tt_embedding", ttm, rows)
    dtype, device = cores[0].dtype, cores[0].device
    shape = tuple(rows.shape) + (cols,)
    if rows.numel() == 0:
        return torch.zeros(shape, dtype=dtype, device=device)
    rows1d = rows.reshape(-1)
    if device.type == "cpu":
        return _hostops.tt_lookup_chain(cores, rows1d).reshape(shape)
    ops = ops_for(cores[0].detach())
    if not _wants_grad(cores):
        return ops.tt_lookup_chain(cores, rows1d).reshape(shape)
    return autodiff.tt_rows(cores, rows1d).reshape(shape)


def tt_embedding_bag(ttm: TTMatrix, rows, offsets=None, per_sample_weights: Optional[torch.Tensor] = None,
                     mode: str = "sum") -> torch.Tensor:
    """The sum or mean of a few rows of ``ttm.torch()`` per bag -> ``[B, cols]``, differentiable in the cores on every device;
    ``torch.nn.functional.embedding_bag``'s conventions.  ``rows`` is 2-D ``[B, L]`` with ``offsets=None`` (bags of ``L``), or 1-D
    ``[P]`` with ``offsets`` (int32 / int64 ``[B]`` on the cores' device: the starts of the bags, non-decreasing, ``offsets[0] ==
    0``; no ``include_last_offset``).  ``mode``: ``"sum"`` or ``"mean"`` (an empty bag gives a row of zeros in both).
    ``per_sample_weights``: a tensor of the shape of ``rows`` in the cores' dtype on their device, with ``"sum"`` only; its
    gradient is not implemented on the device (``NotImplementedError`` when it requires grad under grad mode).  ``ValueError`` for
    anything else, ``IndexError`` for a row outside the matrix.  One host synchronisation on the device: the out-of-range word,
    read together with the check of the offsets."""
    who = "tt_embedding_bag"
    if mode not in ("sum", "mean"):
        raise ValueError("{}: mode must be 'sum' or 'mean', got {!r}".format(who, mode))
    cores, rows, cols = lookup_operands(who, ttm, rows)
    dtype, device = cores[0].dtype, cores[0].device
    if rows.dim() == 2:
        if offsets is not None:
            raise ValueError("{}: 2-D rows are bags of equal length and take no offsets".format(who))
        B, P = int(rows.shape[0]), int(rows.numel())
        seg = torch.arange(B + 1, dtype=torch.int64, device=device) * int(rows.shape[1])
        bad = None
    elif rows.dim() == 1:
        if offsets is None:
            raise ValueError("{}: 1-D rows need the offsets of the bags".format(who))
        if not isinstance(offsets, torch.Tensor):
            offsets = torch.as_tensor(offsets)
            if offsets.dtype in (torch.int32, torch.int64):
                offsets = offsets.to(device)
        if offsets.dtype not in (torch.int32, torch.int64) or offsets.dim() != 1:
            raise ValueError("{}: the offsets must be a 1-D int32 or int64 tensor, got {} of {} dimensions".format(
                who, offsets.dtype, offsets.dim()))
        if offsets.device != device:
            raise ValueError("{}: the matrix and the offsets must be on the same device".format(who))
        B, P = int(offsets.shape[0]), int(rows.shape[0])
        seg = torch.cat([offsets.to(torch.int64), torch.full((1,), P, dtype=torch.int64, device=device)])
        # starts at 0, never decreases; the appended P catches a start beyond the rows
        bad = (seg[0] != 0) | (seg[1:] < seg[:-1]).any()
    else:
        raise ValueError("{}: the rows must be 1-D (with offsets) or 2-D, got {} dimensions".format(who, rows.dim()))
    weights = None
    if per_sample_weights is not None:
        w = per_sample_weights
        if not isinstance(w, torch.Tensor) or tuple(w.shape) != tuple(rows.shape) or w.dtype != dtype or w.device != device:
            raise ValueError("{}: per_sample_weights must be a tensor of the shape of the rows in the cores' dtype on their "
                             "device".format(who))
        if mode != "sum":
            raise ValueError("{}: per_sample_weights go with mode 'sum' only".format(who))
        if device.type != "cpu" and torch.is_grad_enabled() and w.requires_grad:
            raise NotImplementedError("tntorch_amd: the gradient of per_sample_weights is not implemented on the device; detach "
                                      "them or use CPU tensors")
        weights = w.reshape(-1)
    rows1d = rows.reshape(-1)
    lengths = (seg[1:] - seg[:-1]).clamp(min=1).to(dtype) if mode == "mean" else None
    if device.type == "cpu" or P == 0:
        if bad is not None and bool(bad):
            raise ValueError("{}: the offsets must start at 0, not decrease and not pass the number of rows".format(who))
        if P == 0:
            return torch.zeros((B, cols), dtype=dtype, device=device)
        out = _hostops.segment_sum(_hostops.tt_lookup_chain(cores, rows1d), seg, weights)
        return out if lengths is None else out / lengths[:, None]
    ops_for(cores[0].detach())
    return autodiff.tt_rows(cores, rows1d, seg, weights.contiguous() if weights is not None else None, lengths, bad)

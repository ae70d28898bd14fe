"""NumPy-style indexing of ``Tensor`` (tensor.py:1019-1434): ints, slices, ``None``, one ``Ellipsis`` and index arrays.

The key is normalised as in the reference (``_process_key``, tensor.py:1019-1056; a 2-D ``[P, N]`` array is split into its
columns, tensor.py:1086-1093), then walked mode by mode in the cores' ``[B, r, I, r']`` layout (``B = 1`` for non-batch trains):

- a slice keeps the core, sliced along ``I`` (or keeps a Tucker core and slices its factor ``Us[n]``);
- a run of ints is a ``P = 1`` chain of ``[B, r, r']`` slices, multiplied together (``ops.mm``) and joined into the next
  core that is emitted -- or, at the end of the key, into the last one; an all-int key returns the 0-d value (the sum over
  boundary ranks above 1, tensor.py:1419-1422);
- a contiguous block of index arrays becomes one ``[r_a, P, r_b]`` core (``ops.gather_chain``: ``ttr_gather_chain`` on the
  device), with a preceding int chain folded into its first core;
- ``None`` inserts an identity core ``[r, 1, r]``.

Ints and index arrays on a Tucker mode contract the factor into the core first.  The batch dimension of a batch train is
selected up front.  CPU cores run torch ops (the host mirror); device cores only go through ``ttr_gemm`` and
``ttr_gather_chain`` plus data movement (slicing, ``reshape``), and device index tensors are validated on the device.

Device cores or factors that require grad (with grad mode on) take ``autodiff.getitem`` instead: index arrays on the first modes
and slices on the rest are differentiable there, every other key raises ``NotImplementedError``.
"""

from __future__ import annotations

from typing import Any, List, Optional

import numpy as np
import torch

from ._dispatch import ops_for


def _process_key(ndim: int, key) -> list:
    """tensor.py:1019-1056: one entry per dimension (batch dimension included), Ellipsis expanded, slices appended."""
    if isinstance(key, torch.Tensor) and key.dim() == 0:
        key = (key,)
    if not hasattr(key, "__len__"):
        key = (key,)
    if isinstance(key, (torch.Tensor, np.ndarray)):  # one index array on the first dimension
        key = [key]
    elif isinstance(key, tuple):
        key = list(key)
    elif any(not np.isscalar(k) for k in key):  # a list of per-dimension entries
        key = list(key)
    else:  # a list of scalars is one index array
        key = [key]
    nonecount = sum(1 for k in key if k is None)
    for i in range(len(key)):
        if key[i] is Ellipsis:
            key = key[:i] + [slice(None)] * (ndim - (len(key) - nonecount) + 1) + key[i + 1:]
            break
    if any(k is Ellipsis for k in key):
        raise IndexError("Only one ellipsis is allowed, at most")
    if ndim - (len(key) - nonecount) < 0:
        raise IndexError("Too many index entries {} vs {}".format(ndim, len(key) - nonecount))
    return key + [slice(None)] * (ndim - (len(key) - nonecount))


def _kind(k) -> str:
    if isinstance(k, torch.Tensor) and k.dim() == 0:
        return "int"
    if hasattr(k, "__len__"):
        return "index"
    if k is None:
        return "none"
    if isinstance(k, (int, np.integer)):
        return "int"
    if isinstance(k, slice):
        return "slice"
    raise IndexError(f"unsupported index entry {k!r}")


def _check_int(k, size: int) -> int:
    k = int(k)
    if not -size <= k < size:
        raise IndexError(f"index {k} is out of bounds for a mode of size {size}")
    return k


def _index_column(k, device: torch.device) -> torch.Tensor:
    """An index array as a 1-D integer tensor next to the cores.  Device tensors stay where they are (validated by the kernel);
    on CPU cores torch's own indexing raises IndexError."""
    if isinstance(k, torch.Tensor):
        if k.dtype not in (torch.int32, torch.int64):
            k = k.long()
        if device.type == "cpu":
            k = k.cpu()
        return k.to(device).reshape(-1)
    return torch.as_tensor(np.asarray(k, dtype=np.int64).reshape(-1), device=device)


def getitem(t, key: Any):
    from .tensor import Tensor, _not_in_scope

    if isinstance(key, Tensor):
        _not_in_scope("indexing with a mask Tensor (gather tn.accepted_inputs(mask) instead: t[tn.accepted_inputs(mask)])")
    nb = 1 if t.batch else 0
    if any(c.dim() != nb + 3 for c in t.cores):
        _not_in_scope("indexing CP cores")
    if (isinstance(key, torch.Tensor) and key.dim() == 2) or (isinstance(key, np.ndarray) and key.ndim == 2):
        key = [key[:, col] for col in range(key.shape[1])]  # tensor.py:1086-1093
    key = _process_key(len(t.shape), key)

    from . import autodiff

    if autodiff.wants_grad(t):  # device parameters that require grad: the differentiable route, or a refusal
        return autodiff.getitem(t, key)
    c4, Us = t._norm4(), t._norm_us()
    device = c4[0].device
    ops = ops_for(c4[0])

    batch_int = False
    if t.batch:  # the batch dimension, selected up front (tensor.py:1262-1275, 1308-1319, 1381-1384)
        k0, key = key[0], key[1:]
        kind0 = _kind(k0)
        if kind0 == "none":
            raise ValueError("Cannot change batch dimension")
        if kind0 == "int":
            b = _check_int(k0, c4[0].shape[0])
            sel = slice(b, b + 1 if b != -1 else None)
            batch_int = True
        elif kind0 == "slice":
            sel = k0
        else:  # a selection of trains, not point evaluation: the (host-side) batch list is checked on the host
            sel = torch.as_tensor(k0.cpu() if isinstance(k0, torch.Tensor) else np.asarray(k0), dtype=torch.int64).reshape(-1)
            B = c4[0].shape[0]
            if len(sel) and (sel.min() < -B or sel.max() >= B):
                raise IndexError(f"batch index out of range for {B} trains")
            sel = sel.to(device)
            if any(_kind(k) == "index" for k in key):
                raise ValueError("Advanced indexing is prohibited for batch dimension")
        c4 = [c[sel] for c in c4]
        Us = [None if U is None else U[sel] for U in Us]

    cores: List[torch.Tensor] = []
    out_us: List[Optional[torch.Tensor]] = []
    pend: Optional[torch.Tensor] = None  # int chain [B, r_a, r_b]
    block, cols = [], []                 # pending index-array block
    idx_done = False
    n = 0

    def join_left(core4):
        """pend [B, a, r] x core [B, r, I, r'] -> [B, a, I, r']."""
        Bt, r, I, r1 = core4.shape
        return ops.mm(pend, core4.reshape(Bt, r, I * r1)).reshape(Bt, pend.shape[1], I, r1)

    def emit(core4, U=None):
        nonlocal pend
        if pend is not None:
            core4 = join_left(core4)
            pend = None
        cores.append(core4)
        out_us.append(U)

    def flush():
        nonlocal pend, idx_done
        if not block:
            return
        first = block[0]
        if pend is not None:
            first = join_left(first)
            pend = None
        cores.append(ops.gather_chain([first] + block[1:], cols))
        out_us.append(None)
        block.clear()
        cols.clear()
        idx_done = True

    def absorbed(m):
        return c4[m] if Us[m] is None else ops.mode_mul(c4[m], Us[m])

    for k in key:
        kind = _kind(k)
        if kind == "none":
            flush()
            r = c4[n].shape[1] if n < len(c4) else c4[-1].shape[-1]
            eye = torch.eye(r, dtype=c4[0].dtype, device=device)
            emit(eye[None, :, None, :].expand(c4[0].shape[0], r, 1, r).contiguous())
        elif kind == "slice":
            flush()
            if Us[n] is None:
                emit(c4[n][:, :, k, :])
            else:
                emit(c4[n], Us[n][:, k, :])
            n += 1
        elif kind == "index":
            if idx_done:
                raise IndexError("All index arrays must appear contiguously")
            col = _index_column(k, device)
            if block and len(col) != len(cols[0]):
                raise ValueError("Index arrays must have the same length")
            block.append(absorbed(n))
            cols.append(col)
            n += 1
        else:  # int
            flush()
            I = t.shape[n + nb]
            i = _check_int(k, I)
            if Us[n] is None:
                M = c4[n][:, :, i, :]
            else:
                M = ops.mode_mul(c4[n], Us[n][:, i:i + 1 if i != -1 else None, :])[:, :, 0, :]
            pend = M if pend is None else ops.mm(pend, M)
            n += 1
    flush()

    if pend is not None:
        if not cores:  # all ints: a value (tensor.py:1419-1422)
            if not t.batch and pend.numel() > 1:
                return torch.sum(pend)
            return torch.squeeze(pend)
        Bt, a, I, r = cores[-1].shape
        cores[-1] = ops.mm(cores[-1].reshape(Bt, a * I, r), pend).reshape(Bt, a, I, pend.shape[-1])
    if t.batch and not batch_int:
        return Tensor(cores, Us=out_us, batch=True)
    return Tensor([c[0] for c in cores], Us=[None if U is None else U[0] for U in out_us], batch=False)

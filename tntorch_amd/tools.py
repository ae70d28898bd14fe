"""Unfoldings of TT cores / dense tensors -- the layout contract of the hot path -- and the rounding tree.

Mirror of ``tntorch/tools.py:211-258`` (same names, arguments and results), ``convolve`` (tools.py:579-647) and ``mask``
(tools.py:333-359).  All three are
pure ``reshape``/``permute`` views: a core ``[r0, I, r1]`` is row-major, so its left
unfolding has row index ``r0*I + i`` and its right unfolding column index ``i*R1 + r1`` --
exactly the addressing the HIP kernels use (no data movement on either side).
"""

import time

import numpy as np
import torch

__all__ = ["meshgrid", "unfolding", "right_unfolding", "left_unfolding", "reduce", "shift_mode", "convolve", "mask"]


def meshgrid(*axes, batch=False):
    """tools.py:135-166: N tensors of N dimensions (rank 1 each), the n-th varying along mode n.  Axes are ints (``arange``) or
    vectors, cast to the default dtype; the cores live on the device of the first axis."""
    from .tensor import Tensor

    device = None
    if not hasattr(axes, "__len__"):
        axes = [axes]
    if hasattr(axes[0], "__len__"):
        axes = axes[0]
    if hasattr(axes[0], "device"):
        device = axes[0].device
    axes = list(axes)
    N = len(axes)
    for n in range(N):
        if not hasattr(axes[n], "__len__"):
            axes[n] = torch.arange(axes[n], dtype=torch.get_default_dtype())
    tensors = []
    for n in range(N):
        cores = [torch.ones(1, len(ax), 1).to(device) for ax in axes]
        if isinstance(axes[n], torch.Tensor):
            cores[n] = axes[n].type(torch.get_default_dtype())
        else:
            cores[n] = torch.tensor(np.asarray(axes[n]), dtype=torch.get_default_dtype())
        cores[n] = cores[n][None, :, None].to(device)
        tensors.append(Tensor(cores, device=device, batch=batch))
    return tensors


def unfolding(data: torch.Tensor, n: int, batch: bool = False) -> torch.Tensor:
    """Mode-``n`` unfolding of a dense tensor (tools.py:211-228)."""
    if batch:
        order = [0, n + 1] + list(range(1, n + 1)) + list(range(n + 2, data.dim()))
        return data.permute(order).reshape([data.shape[0], data.shape[n + 1], -1])
    order = [n] + list(range(n)) + list(range(n + 1, data.dim()))
    return data.permute(order).reshape([data.shape[n], -1])


def right_unfolding(core: torch.Tensor, batch: bool = False) -> torch.Tensor:
    """``[r0, I, r1] -> [r0, I*r1]`` (tools.py:231-243)."""
    if batch:
        return core.reshape([core.shape[0], core.shape[1], -1])
    return core.reshape([core.shape[0], -1])


def left_unfolding(core: torch.Tensor, batch: bool = False) -> torch.Tensor:
    """``[r0, I, r1] -> [r0*I, r1]`` (tools.py:246-258)."""
    if batch:
        return core.reshape([core.shape[0], -1, core.shape[-1]])
    return core.reshape([-1, core.shape[-1]])


def reduce(ts, function, eps=0, rmax=np.iinfo(np.int32).max, algorithm="svd", verbose=False, **kwargs):
    """Fold a sequence (or generator) of tensors with ``function`` (``operator.add``, ``tn.cat`` ...), rounding after
    every combination so that no intermediate exceeds ``rmax`` / ``eps`` -- same contract as tools.py:460-512.

    The combinations form a balanced tree built on the fly like a binary counter: ``slots[h]`` holds the rounded result
    of a complete group of 2**h consecutive elements (or nothing); a new element enters at height 0 and, like a carry,
    merges upwards while the slot at its height is occupied.  Operands of a merge therefore always cover equally many
    elements (similar ranks meet), at most log2(len) partial results are alive, and ``function`` always receives the
    EARLIER group first (order matters for e.g. concatenation).  At the end the remaining groups are merged from the
    oldest (highest) to the newest.
    """
    import operator

    from .round import round as _round
    from .tensor import Tensor

    def merge(older, newer):
        if function is operator.add and not kwargs:
            # add-then-round fused: the concatenated cores of the sum are never materialised (device TT tensors)
            fused = Tensor._round_of_sum(older, newer, eps=eps, rmax=rmax, algorithm=algorithm)
            if fused is not None:
                return fused
        return _round(function(older, newer, **kwargs), eps=eps, rmax=rmax, algorithm=algorithm)

    slots = []
    started = time.time()
    for count, item in enumerate(ts):
        if verbose and count % 100 == 0:
            print("reduce: element {}, time={:g}".format(count, time.time() - started))
        height = 0
        while height < len(slots) and slots[height] is not None:
            item = merge(slots[height], item)
            slots[height] = None
            height += 1
        if height == len(slots):
            slots.append(item)
        else:
            slots[height] = item
    groups = [g for g in reversed(slots) if g is not None]
    if not groups:
        raise ValueError("reduce() needs at least one tensor")
    result = groups[0]
    for g in groups[1:]:
        result = merge(result, g)
    return result


def shift_mode(t, n, shift, eps=1e-3):
    """Move mode ``n`` of a tensor train ``shift`` positions to the right (``shift > 0``) or left, in place on the core list
    -- same contract as tools.py:650-697: the train is made ``n``-orthogonal, then every exchange of two neighbouring
    modes contracts the two cores, swaps the mode axes and splits the result again by ``truncated_svd`` (relative error
    ``eps / sqrt(|shift|)`` per exchange, or ``eps='same'``: the old bond rank is the cap).  On device tensors the
    contraction is one MFMA GEMM and the split the Gram / eigensolver / projection kernels of the rounding sweep.
    """
    from ._dispatch import ops_for
    from .round import truncated_svd

    N = t.dim()
    assert 0 <= n + shift < N
    if shift == 0:
        return t
    if t.batch:
        raise NotImplementedError("shift_mode: batched tensors are not supported (the reference indexes core.shape[0] as a rank)")
    if any(U is not None for U in t.Us):
        t = t.decompress_tucker_factors(_clone=False)
    if isinstance(eps, str):
        if eps != "same":
            raise ValueError("Relative error '{}' not recognized".format(eps))
    elif not eps >= 0:
        raise ValueError("Relative error '{}' not recognized".format(eps))
    t.orthogonalize(n)
    cores = t._norm4()  # [1, r0, I, r1] views (CP factors become TT cores, as the reference's orthogonalize does)
    sign = 1 if shift > 0 else -1
    for i in range(n, n + shift, sign):
        c1, c2, left_ortho = (i, i + 1, True) if sign == 1 else (i - 1, i, False)
        _, R1, I1, R2 = cores[c1].shape
        _, _, I2, R3 = cores[c2].shape
        sc = ops_for(cores[c1]).merge_swap(cores[c1], cores[c2])[0]  # [R1*I2, I1*R3]
        if isinstance(eps, str):
            left, right = truncated_svd(sc, eps=0, rmax=R2, left_ortho=left_ortho)
        else:
            left, right = truncated_svd(sc, eps=eps / np.sqrt(np.abs(shift)), left_ortho=left_ortho)
        newR2 = left.shape[1]
        cores[c1] = left.reshape(1, R1, I2, newR2)
        cores[c2] = right.reshape(1, newR2, I1, R3)
    t.cores = t._denorm(cores)
    return t


# the keyword arguments of tn.cross that the reference's convolve hands on: accepted and ignored (nothing is cross-approximated)
_CROSS_KWARGS = frozenset(["ranks_tt", "kickrank", "max_iter", "val_size", "verbose", "return_info", "record_samples", "device",
                           "suppress_warnings", "detach_evaluations", "function_arg"])


def convolve_window(I, J, mode):
    """(lo, K): the entries lo .. lo + K - 1 of the full convolution (I + J - 1 entries) of modes of sizes I and J that
    ``np.convolve`` returns for ``mode``."""
    k, m = min(I, J), max(I, J)
    if mode == "full":
        return 0, I + J - 1
    if mode == "same":
        return (k - 1) // 2, m
    if mode == "valid":
        return k - 1, m - k + 1
    raise ValueError("convolve: mode must be 'full', 'same' or 'valid', got {!r}".format(mode))


def convolve(t1, t2, mode="full", eps=1e-6, rmax=None, algorithm="svd", **kwargs):
    """N-D convolution of two tensors (tools.py:579-647), computed exactly: the convolution of two trains is a train whose core
    ``n`` is the mode-wise convolution of the two cores, slice-wise Kronecker in the ranks,

        C_n[r1 S1 + s1, k, r2 S2 + s2] = sum_i A_n[r1, i, r2] B_n[s1, k + lo - i, s2]

    (one ``ttr_core_convolve`` launch per mode on device tensors; only the window of ``mode`` is computed).  Its ranks are the
    products ``r s``; one ``round_tt(eps=eps or 0, rmax=rmax, algorithm=algorithm)`` brings them down, so ``eps`` bounds the
    relative Frobenius error.  ``eps=None`` and ``rmax=None``: the exact train is returned unrounded.  When every rank of one
    input is 1 (a separable kernel) the ranks do not grow and, for ``rmax=None``, nothing is rounded.  Tucker factors are
    contracted in first, as the reference does.  ``mode``: ``'full'`` (``I + J - 1`` per mode), ``'same'`` (``max(I, J)``) or
    ``'valid'`` (``max(I, J) - min(I, J) + 1``), ``np.convolve``'s windows per mode.

    Unlike the reference (which multiplies the FFTs of the cores with three TT-cross runs on complex trains):
      - the result is deterministic, real, and on the inputs' device in their dtype (fp32 or fp64);
      - ``eps`` is ``round_tt``'s bound on the relative error, not cross's stopping criterion; the other keyword arguments of
        ``tn.cross`` are accepted and ignored, any other keyword raises TypeError;
      - ``'same'`` with an even smaller size starts at ``(k - 1) // 2`` as numpy does (the reference at ``k // 2``), and
        ``'valid'`` with a smaller size of 1 returns the whole mode (the reference's slice ``[k-1 : -(k-1)]`` is empty there);
      - different numbers of modes, devices or dtypes, batched inputs, an unknown ``mode`` and non-Tensor arguments raise
        ValueError, CP cores NotImplementedError.
    """
    from ._dispatch import ops_for
    from .tensor import Tensor, _not_in_scope

    unknown = sorted(set(kwargs) - _CROSS_KWARGS)
    if unknown:
        raise TypeError("convolve() got an unexpected keyword argument {!r}".format(unknown[0]))
    for t in (t1, t2):
        if not isinstance(t, Tensor):
            raise ValueError("convolve: expected a tntorch_amd.Tensor, got {}".format(type(t).__name__))
        if t.batch:
            raise ValueError("Batched tensors are not supported.")
        if any(c.dim() == 2 for c in t.cores):
            _not_in_scope("convolve of CP cores")
    N = t1.dim()
    if t2.dim() != N:
        raise ValueError("convolve: the tensors have {} and {} modes".format(N, t2.dim()))
    c1, c2 = t1.cores[0], t2.cores[0]
    if c1.device != c2.device or c1.dtype != c2.dtype:
        raise ValueError("convolve: the tensors live on {} ({}) and {} ({})".format(c1.device, c1.dtype, c2.device, c2.dtype))
    windows = [convolve_window(I, J, mode) for I, J in zip(t1.shape, t2.shape)]
    a = [c[0].contiguous() for c in t1._absorbed4()]
    b = [c[0].contiguous() for c in t2._absorbed4()]
    ops = ops_for(a[0])
    out = Tensor([ops.core_convolve(x, y, lo, K) for x, y, (lo, K) in zip(a, b, windows)])
    separable = all(x.shape[0] == 1 and x.shape[2] == 1 for x in a) or all(y.shape[0] == 1 and y.shape[2] == 1 for y in b)
    if (eps is None and rmax is None) or (separable and rmax is None):
        return out
    out.round_tt(eps=eps or 0, rmax=rmax, algorithm=algorithm)
    return out


def mask(t, mask):
    """Masks a tensor (tools.py:333-359): the element-wise product ``t * mask``, with the mask's slices matched by their meaning --
    slice ``j`` of mode ``n`` of ``t`` meets slice ``t.idxs[n][j]`` of the mask, clamped to the mask's size (identity indexing
    unless ``t`` carries ``idxs``).  The selection is made on the mask's Tucker factor where it has one.  Everything runs on
    ``t``'s device; the product is ``Tensor.__mul__`` (one ``core_kron`` per mode).

    :param t: input :class:`Tensor`
    :param mask: a mask :class:`Tensor`

    :return: masked :class:`Tensor`
    """
    from .tensor import Tensor

    for x, what in ((t, "t"), (mask, "mask")):
        if not isinstance(x, Tensor):
            raise ValueError("mask: {} must be a tntorch_amd.Tensor, got {}".format(what, type(x).__name__))
        if x.batch:
            raise ValueError("Batched tensors are not supported.")
    if mask.dim() != t.dim():
        raise ValueError("mask: the tensor has {} modes, the mask {}".format(t.dim(), mask.dim()))
    device, dtype = t.cores[0].device, t.cores[0].dtype
    cores, Us = [], []
    for n in range(t.dim()):
        idx = t.idxs[n] if torch.is_tensor(t.idxs[n]) else torch.as_tensor(np.asarray(t.idxs[n]))
        idx = idx.to(device).long().clamp(max=mask.shape[n] - 1)
        core = mask.cores[n].to(device=device, dtype=dtype)
        if mask.Us[n] is None:
            cores.append(core[..., idx, :])
            Us.append(None)
        else:
            cores.append(core)
            Us.append(mask.Us[n].to(device=device, dtype=dtype)[idx, :])
    return t * Tensor(cores, Us=Us)

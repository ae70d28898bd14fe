"""Array-like manipulations, multilinear algebra, the unfoldings of TT cores / dense tensors -- the layout contract of the hot
path -- and the rounding tree.

Mirror of ``tntorch/tools.py``: the array tools (tools.py:14-208: ``squeeze``, ``unsqueeze``, ``cat``, ``transpose``, ``meshgrid``,
``flip``, ``unbind``), the unfoldings (tools.py:211-258), ``ttm`` (tools.py:266-325), ``mask`` (tools.py:333-359),
``generate_basis`` (tools.py:427-457), ``reduce`` (tools.py:460-512), ``pad`` (tools.py:515-576) and ``convolve``
(tools.py:579-647), and ``sample`` (tools.py:362-407), with the names, arguments and results of the reference; what differs is
listed in each docstring.  ``hash`` is out of scope.  The array tools follow the input's device and dtype (fp32 or fp64) and never modify their inputs;
on device tensors a matrix factor goes through the MFMA GEMM (``mode_mul``), a vector factor through ``ttr_mode_reduce``, and
everything else is slicing and copies of cores.

The unfoldings are pure ``reshape``/``permute`` views: a core ``[r0, I, r1]`` is row-major, so its left
unfolding has row index ``r0*I + i`` and its right unfolding column index ``i*R1 + r1`` --
exactly the addressing the HIP kernels use (no data movement on either side).
"""

import operator
import time

import numpy as np
import torch

__all__ = ["meshgrid", "unfolding", "right_unfolding", "left_unfolding", "reduce", "shift_mode", "convolve", "mask", "squeeze",
           "unsqueeze", "cat", "transpose", "flip", "unbind", "ttm", "generate_basis", "pad", "sample"]


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


# ---------------------------------------------------------------------------------------------- array tools (tools.py:14-208, 266-325, 427-457, 515-576)
def _check_array_tensor(t, what):
    from .tensor import Tensor, _not_in_scope

    if not isinstance(t, Tensor):
        raise ValueError("{}: expected a tntorch_amd.Tensor, got {}".format(what, type(t).__name__))
    if t.batch:
        raise ValueError("Batched tensors are not supported.")
    if any(c.dim() == 2 for c in t.cores):
        _not_in_scope("{} of CP cores".format(what))


def _array_dims(dim, N, what, unique=True):
    """``dim`` (an int or a sequence of ints, negative ones counted from the end) as a list of modes of an ``N``-mode tensor."""
    dims = list(dim) if hasattr(dim, "__len__") or isinstance(dim, range) else [dim]
    out = []
    for d in dims:
        if isinstance(d, bool) or int(d) != d or not -N <= d < N:
            raise ValueError("{}: dim {!r} out of range for a tensor of {} modes".format(what, d, N))
        out.append(int(d) % N)
    if unique and len(set(out)) != len(out):
        raise ValueError("{}: dim {!r} repeats a mode".format(what, dim))
    return out


def squeeze(t, dim=None):
    """Removes singleton dimensions (tools.py:14-34), through ``Tensor.__getitem__`` as the reference does.

    :param t: input :class:`Tensor`
    :param dim: which dim(s) to delete.  By default, all that have size 1

    :return: another :class:`Tensor`, without dummy (singleton) indices; when no mode is left (every mode was a singleton), what
        indexing with all ints returns: a 0-dim torch tensor on ``t``'s device

    Unlike the reference: a ``dim`` out of range or repeated and a mode whose size is not 1 raise ValueError (an ``assert``
    there), batched tensors ValueError, CP cores NotImplementedError.
    """
    _check_array_tensor(t, "squeeze")
    shape = t.shape
    if dim is None:
        dims = [n for n, sh in enumerate(shape) if sh == 1]
    else:
        dims = _array_dims(dim, t.dim(), "squeeze")
    for d in dims:
        if shape[d] != 1:
            raise ValueError("squeeze: mode {} has size {}, not 1".format(d, shape[d]))
    idx = [slice(None)] * t.dim()
    for d in dims:
        idx[d] = 0
    return t[tuple(idx)]


def unsqueeze(t, dim):
    """Inserts singleton dimensions at specified positions (tools.py:37-53), through ``Tensor.__getitem__``.

    :param t: input :class:`Tensor`
    :param dim: int or list of ints: positions in the RESULT (``t.dim() + len(dim)`` modes)

    :return: a :class:`Tensor` with dummy (singleton) dimensions inserted at the positions given by ``dim``

    Unlike the reference: a ``dim`` out of range or repeated raises ValueError, batched tensors ValueError, CP cores
    NotImplementedError.
    """
    _check_array_tensor(t, "unsqueeze")
    count = len(dim) if hasattr(dim, "__len__") else 1
    dims = _array_dims(dim, t.dim() + count, "unsqueeze")
    idx = [slice(None)] * (t.dim() + count)
    for d in dims:
        idx[d] = None
    return t[tuple(idx)]


def unbind(t, dim):
    """Slices a tensor along a dimension and returns the slices as a sequence, like PyTorch's ``unbind()`` (tools.py:193-208).

    :param t: input :class:`Tensor`
    :param dim: an int

    :return: a list of :class:`Tensor` (0-dim torch tensors for a one-mode ``t``), as many as ``t.shape[dim]``

    Unlike the reference: a ``dim`` out of range raises ValueError, batched tensors ValueError, CP cores NotImplementedError.
    """
    _check_array_tensor(t, "unbind")
    (d,) = _array_dims([dim], t.dim(), "unbind")
    N = t.dim()
    return [t[tuple([slice(None)] * d + [sl] + [slice(None)] * (N - 1 - d))] for sl in range(t.shape[d])]


def cat(*ts, dim):
    """Concatenate two or more tensors along a given dim, similarly to PyTorch's ``cat()`` (tools.py:56-104).

    :param ts: a list of :class:`Tensor` (or the tensors themselves)
    :param dim: an int

    :return: a :class:`Tensor` of the same shape as all tensors in the list, except along ``dim`` where it has the sum of shapes.
        One tensor: a clone of it

    The result is built directly, one allocation per core: the cores off ``dim`` are block-diagonal in the ranks, at ``dim`` block
    ``k`` sits in tensor ``k``'s rank rows, its own index range and its rank columns, and the first and the last core are
    concatenated along their free rank -- the TT ranks add.  (The reference makes K zero-padded clones and K - 1 sums: the same
    tensor.)  When every input has a Tucker factor on ``dim`` the factors are stacked block-wise (``[sum I_k, sum S_k]``) under a
    core that is block-diagonal in the Tucker index too; otherwise the factors on ``dim`` are contracted into the cores.  Factors
    off ``dim`` are contracted in, as ``+`` does.

    Unlike the reference: the result lives on the inputs' device in their dtype (the reference allocates default-dtype CPU zeros:
    fp64 cores raise ``expected scalar type Float but found Double`` there unless the default dtype is fp64); a ``dim`` out of
    range, different numbers of modes, devices or dtypes and batched tensors raise ValueError, CP cores NotImplementedError.
    """
    from ._dispatch import ops_for
    from .tensor import Tensor

    if len(ts) == 1 and isinstance(ts[0], (list, tuple)):
        ts = ts[0]
    ts = list(ts)
    if not ts:
        raise ValueError("cat: needs at least one tensor")
    for t in ts:
        _check_array_tensor(t, "cat")
    if len(ts) == 1:
        return ts[0].clone()
    N = ts[0].dim()
    c0 = ts[0].cores[0]
    for t in ts[1:]:
        if t.dim() != N:
            raise ValueError("cat: the tensors have {} and {} modes".format(N, t.dim()))
        if t.cores[0].device != c0.device or t.cores[0].dtype != c0.dtype:
            raise ValueError("cat: the tensors live on {} ({}) and {} ({})".format(c0.device, c0.dtype, t.cores[0].device, t.cores[0].dtype))
    (d,) = _array_dims([dim], N, "cat")
    if any(t.shape[n] != ts[0].shape[n] for t in ts[1:] for n in range(N) if n != d):
        raise ValueError("To concatenate tensors, all must have the same shape along all but the given dim")
    stacked = all(t.Us[d] is not None for t in ts)
    per = []   # per tensor: cores [r, I, r'] with every factor contracted in, but the one on `d` when all have one
    for t in ts:
        c4, Us3 = t._norm4(), t._norm_us()
        per.append([c4[n][0] if Us3[n] is None or (n == d and stacked) else ops_for(c4[n]).mode_mul(c4[n], Us3[n])[0] for n in range(N)])
    cores = []
    for n in range(N):
        blocks = [p[n] for p in per]
        rows = blocks[0].shape[0] if n == 0 else sum(b.shape[0] for b in blocks)
        cols = blocks[0].shape[2] if n == N - 1 else sum(b.shape[2] for b in blocks)
        mid = sum(b.shape[1] for b in blocks) if n == d else blocks[0].shape[1]
        if (n == 0 and any(b.shape[0] != rows for b in blocks)) or (n == N - 1 and any(b.shape[2] != cols for b in blocks)):
            raise ValueError("cat: the tensors have different boundary ranks")
        core = c0.new_zeros((rows, mid, cols))
        r = i = c = 0
        for b in blocks:
            rs = slice(None) if n == 0 else slice(r, r + b.shape[0])          # the first core keeps its boundary rank rows,
            cs = slice(None) if n == N - 1 else slice(c, c + b.shape[2])      # the last one its columns
            core[rs, slice(i, i + b.shape[1]) if n == d else slice(None), cs] = b
            r, i, c = r + b.shape[0], i + b.shape[1], c + b.shape[2]
        cores.append(core)
    Us = [None] * N
    if stacked:
        U = c0.new_zeros((sum(t.Us[d].shape[0] for t in ts), sum(t.Us[d].shape[1] for t in ts)))
        i = s = 0
        for t in ts:
            I, S = t.Us[d].shape
            U[i:i + I, s:s + S] = t.Us[d]
            i, s = i + I, s + S
        Us[d] = U
    return Tensor(cores, Us=Us)


def transpose(t):
    """Inverts the dimension order of a tensor, e.g. I1 x I2 x I3 becomes I3 x I2 x I1 (tools.py:107-132): the cores in reverse
    order, each ``permute(2, 1, 0)`` (made contiguous), with ``Us`` and ``idxs`` reversed.

    :param t: input :class:`Tensor`

    :return: another :class:`Tensor`, indexed by dimensions in inverse order

    Unlike the reference: batched tensors raise ValueError, CP cores NotImplementedError.
    """
    from .tensor import Tensor

    _check_array_tensor(t, "transpose")
    cores = [c.permute(2, 1, 0).contiguous() for c in reversed(t.cores)]
    Us = [None if U is None else U.clone() for U in reversed(t.Us)]
    idxs = None if t._idxs is None else [i.clone() if torch.is_tensor(i) else i for i in reversed(t._idxs)]
    return Tensor(cores, Us=Us, idxs=idxs)


def flip(t, dim):
    """Reverses the order of a tensor along one or several dimensions; see NumPy's or PyTorch's ``flip()`` (tools.py:169-190).  The
    Tucker factor is reversed where the mode has one, else the core.

    :param t: input :class:`Tensor`
    :param dim: an int or list of ints

    :return: another :class:`Tensor` of the same shape

    Unlike the reference: a ``dim`` out of range or repeated raises ValueError, batched tensors ValueError, CP cores
    NotImplementedError.
    """
    _check_array_tensor(t, "flip")
    dims = _array_dims(dim, t.dim(), "flip")
    result = t.clone()
    for d in dims:
        if result.Us[d] is not None:
            result.Us[d] = torch.flip(result.Us[d], [0])
        else:
            result.cores[d] = torch.flip(result.cores[d], [1])
    return result


def ttm(t, U, dim=None, transpose=False):
    """Tensor-times-matrix (TTM) along one or several dimensions (tools.py:266-325).

    :param t: input :class:`Tensor`
    :param U: one or several factors (vectors or matrices)
    :param dim: one or several dimensions.  If None, the first ``len(U)`` dims are assumed
    :param transpose: if False (default) a matrix factor is ``[J, I_n]`` (mode ``n`` is contracted with its second index), else
        ``[I_n, J]``; the transposed factor is not copied (it enters the GEMM as a transposed operand)

    :return: transformed :class:`Tensor`: mode ``n`` has size ``J``

    A matrix factor goes through ``mode_mul`` (one batched MFMA GEMM on device tensors); a mode with a Tucker factor keeps its
    structure (``factor @ Us[n]``, the core is untouched).  A 1-D factor ``[I_n]`` is a row ``[1, I_n]``: the mode stays as a
    singleton, computed by the weighted reduction of the mode axis (``ttr_mode_reduce``: the mode is read once, no M = 1 GEMM) --
    marginalising or integrating a mode is ``tn.squeeze(tn.ttm(t, weights, dim))``.

    Unlike the reference: the factors are taken to ``t``'s device and dtype; a ``dim`` out of range or repeated, a number of
    factors other than ``len(dim)`` and a factor whose contracted size is not the mode's raise ValueError (an einsum error there),
    batched tensors ValueError, CP cores NotImplementedError.
    """
    from ._dispatch import ops_for
    from .tensor import Tensor

    _check_array_tensor(t, "ttm")
    if not isinstance(U, (list, tuple)):
        U = [U]
    dims = _array_dims(range(min(len(U), t.dim())) if dim is None else dim, t.dim(), "ttm")
    if len(dims) != len(U):
        raise ValueError("ttm: {} factors for {} modes".format(len(U), len(dims)))
    c0 = t.cores[0]
    shape = t.shape
    cores, Us = [], []
    for n in range(t.dim()):
        core, fac = t.cores[n], t.Us[n]
        if n not in dims:
            cores.append(core.clone())
            Us.append(None if fac is None else fac.clone())
            continue
        M = U[dims.index(n)]
        if not torch.is_tensor(M):
            M = torch.as_tensor(np.asarray(M))
        if M.dim() not in (1, 2):
            raise ValueError("ttm: the factor for mode {} has {} dimensions (1 or 2 expected)".format(n, M.dim()))
        M = M.to(device=c0.device, dtype=c0.dtype)
        contracted = M.shape[0] if (M.dim() == 1 or transpose) else M.shape[1]
        if contracted != shape[n]:
            raise ValueError("ttm: the factor for mode {} contracts {} entries, the mode has {}".format(n, contracted, shape[n]))
        target = core if fac is None else fac[None]   # [r, I, r'] or the factor as [1, I, S]
        ops = ops_for(target)
        if M.dim() == 1:
            out = ops.mode_reduce(target.contiguous(), M.contiguous())[:, None, :]   # [r, 1, r']
        else:
            out = ops.mode_mul(target[None], M[None], trans=bool(transpose))[0]     # [r, J, r']
        if fac is None:
            cores.append(out)
            Us.append(None)
        else:
            cores.append(core.clone())
            Us.append(out[0])
    return Tensor(cores, Us=Us, idxs=t._idxs)


def generate_basis(name, shape, orthonormal=False):
    """Generate a factor matrix whose columns are functions of a truncated basis (tools.py:427-457).

    :param name: 'dct', 'identity', 'legendre', 'chebyshev' or 'hermite'
    :param shape: two integers ``(I, K)``
    :param orthonormal: whether to normalise the columns to unit 2-norm

    :return: an fp64 CPU matrix of ``shape``, as the reference returns (``tn.ttm`` takes it to the tensor's device and dtype)

    ``'dct'`` is the orthonormal DCT-II in closed form, ``U[i, k] = c_k cos(pi (2 i + 1) k / (2 I))`` with ``c_0 = I^-1/2`` and
    ``c_k = (2 / I)^1/2`` (what ``scipy.fftpack.dct(eye(I), norm='ortho')`` returns; this package does not import scipy); the
    polynomial bases are evaluated at ``linspace(-1, 1, I)``.

    Unlike the reference: ``orthonormal=True`` really divides each column by its 2-norm (the reference computes the quotient and
    discards it); an unknown ``name`` raises ValueError for every name (also there), a shape that is not two positive integers too.
    """
    if not hasattr(shape, "__len__") or len(shape) != 2 or int(shape[0]) < 1 or int(shape[1]) < 1:
        raise ValueError("generate_basis: shape must be two positive integers, got {!r}".format(shape))
    I, K = int(shape[0]), int(shape[1])
    if name == "dct":
        i, k = np.arange(I, dtype=np.float64)[:, None], np.arange(K, dtype=np.float64)[None, :]
        U = np.cos(np.pi * (2 * i + 1) * k / (2 * I)) * np.where(k == 0, np.sqrt(1.0 / I), np.sqrt(2.0 / I))
        U[:, I:] = 0   # (the reference's slice has no columns past I; there is no DCT function beyond k = I - 1)
    elif name == "identity":
        U = np.eye(I, K)
    elif name in ("legendre", "chebyshev", "hermite"):
        eval_points = np.linspace(-1, 1, I)
        val = {"legendre": np.polynomial.legendre.legval, "chebyshev": np.polynomial.chebyshev.chebval,
               "hermite": np.polynomial.hermite.hermval}[name]
        U = val(eval_points, np.eye(I, K)).T
    else:
        raise ValueError("Unsupported basis function")
    U = np.ascontiguousarray(U, dtype=np.float64)
    if orthonormal:
        norms = np.sqrt(np.sum(U * U, axis=0))
        U = U / np.where(norms > 0, norms, 1.0)
    return torch.from_numpy(U)


def pad(t, shape, dim=None, fill_value=0):
    """Pad a tensor with a constant value (tools.py:515-576).

    :param t: N-dim input :class:`Tensor`
    :param shape: int or list of ints: the target sizes of the modes ``dim``
    :param dim: int or list of ints (default: all modes)
    :param fill_value: default is 0

    :return: a :class:`Tensor` of size ``shape`` along the indicated modes: ``t`` in the box of its original sizes, ``fill_value``
        everywhere else.  The rows are appended to the Tucker factor where the mode has one, else to the core

    ``fill_value=0`` is the reference's result exactly.  Unlike the reference for ``fill_value != 0``: EVERY entry outside the
    original box equals ``fill_value`` -- the result is the zero-padded train plus ``fill_value`` times (all-ones minus the
    indicator of the box), which raises the TT ranks by at most 2 (Tucker factors are contracted in by that sum); the reference
    writes ``fill_value`` into the first padded core and zeros into the others, so its padded entries are products with the
    neighbouring cores, not the constant.  A target size below the current size, a ``dim`` out of range or repeated and a number of
    sizes other than ``len(dim)`` raise ValueError, batched tensors ValueError, CP cores NotImplementedError.
    """
    from ._dispatch import ops_for
    from .tensor import Tensor

    _check_array_tensor(t, "pad")
    N = t.dim()
    dims = _array_dims(range(N) if dim is None else dim, N, "pad")
    sizes = [int(x) for x in shape] if hasattr(shape, "__len__") else [int(shape)] * len(dims)
    if len(sizes) != len(dims):
        raise ValueError("pad: {} sizes for {} modes".format(len(sizes), len(dims)))
    old = list(t.shape)
    new = list(old)
    for d, sz in zip(dims, sizes):
        if sz < old[d]:
            raise ValueError("pad: target size {} of mode {} is below its size {}".format(sz, d, old[d]))
        new[d] = sz
    cores = [c.clone() for c in t.cores]
    Us = [None if U is None else U.clone() for U in t.Us]
    for d in dims:
        extra = new[d] - old[d]
        if extra == 0:
            continue
        if Us[d] is not None:
            Us[d] = torch.cat([Us[d], Us[d].new_zeros((extra, Us[d].shape[1]))], dim=0)
        else:
            c = cores[d]
            cores[d] = torch.cat([c, c.new_zeros((c.shape[0], extra, c.shape[2]))], dim=1)
    result = Tensor(cores, Us=Us)
    if fill_value == 0 or new == old:
        return result
    c0 = t.cores[0]
    if c0.shape[0] != 1 or t.cores[-1].shape[2] != 1:
        raise ValueError("pad: fill_value != 0 needs boundary ranks 1, got {} and {}".format(c0.shape[0], t.cores[-1].shape[2]))
    # fill_value * (all-ones - box indicator) = fill_value * sum_n [inside before n] [outside at n]: a train of rank 2 over the
    # states "inside so far" / "outside already", with entries 0 and 1 only (nothing cancels inside the box)
    fill = []
    for n in range(N):
        ins = c0.new_zeros(new[n])
        ins[:old[n]] = 1
        core = c0.new_zeros((2, new[n], 2))
        core[0, :, 0] = ins
        core[0, :, 1] = 1 - ins
        core[1, :, 1] = 1
        if n == 0:
            core = core[:1]
        if n == N - 1:
            core = core[:, :, 1:]
        fill.append(core.contiguous())
    fill[0] = ops_for(fill[0]).scale(fill[0], fill_value)
    return result + Tensor(fill)


def _sample_from_thresholds(t, U):
    """The sweep of :func:`sample` for given thresholds ``U`` (fp64 ``[P, N]`` on ``t``'s device, entries in ``[0, 1)``): sample
    ``p`` takes at mode ``mu`` the smallest index whose running conditional mass exceeds ``U[p, mu]`` times the total."""
    from .automata import _cores3

    return _sample_sweep(_cores3(t, "sample"), U)


def _sample_sweep(cores, U):
    from . import _hostops
    from ._dispatch import ops_for

    ops = ops_for(cores[0])
    dev, N = cores[0].device, len(cores)
    if not (isinstance(U, torch.Tensor) and U.dim() == 2 and U.shape[1] == N and U.dtype == torch.float64 and U.device == dev):
        raise ValueError("sample: the thresholds must be an fp64 [P, {}] tensor on the tensor's device".format(N))
    limit = ops.sample_max_rank()
    rmax = max(max(c.shape[0], c.shape[2]) for c in cores)
    if limit is not None and rmax > limit:
        raise ValueError("sample: rank {} is above the limit of {} (ttr_sample_max_rank)".format(rmax, limit))
    P = U.shape[0]
    Xs = torch.empty((P, N), dtype=torch.int64, device=dev)
    if P == 0:
        return Xs
    fibers = ops.sample_fibers(cores)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    L = torch.ones((P, cores[0].shape[0]), dtype=cores[0].dtype, device=dev)
    for mu in range(N):
        L = ops.sample_step(L, fibers[mu], cores[mu], U[:, mu], Xs[:, mu], flag, mu == N - 1)
    word = int(flag.item())                                             # (the one readback of a call)
    if word != 0:
        raise ValueError("sample: {} (flag word {})".format("; ".join(
            text for bit, text in ((_hostops.SAMPLE_ZERO_TOTAL, "a sample met a conditional distribution of zero total mass (the zero tensor, or a "
                                                                    "prefix whose left vector annihilates the next fiber)"),
                                   (_hostops.SAMPLE_NONFINITE, "a conditional total is not finite (NaN or infinity in the cores)"),
                                   (_hostops.SAMPLE_BAD_THRESHOLD, "a threshold lies outside [0, 1)")) if word & bit), word))
    return Xs


def sample(t, P=1, seed=None):
    """Draw ``P`` index vectors, with replacement, from the distribution whose unnormalised mass function is ``t``
    (tools.py:362-407).  The conditional marginal of a mode given the earlier indices is taken in absolute value, as the
    reference takes it; ``t`` does not have to sum to 1.

    What differs from the reference: the result is int64 and lives on ``t``'s device (the reference returns a float32 CPU
    matrix); the thresholds are compared with ``u T`` instead of normalising each row, the left vectors are divided by their
    total ``T`` and the right vectors by their largest magnitude (scales that cancel; without them fp32 underflows after a few
    dozen modes); where rounding leaves no index above the threshold the last index of positive mass is taken; a conditional
    distribution of zero or non-finite total raises ``ValueError`` (the reference divides by zero).  On device tensors each mode is
    one launch of ``ttr_sample_step``: the ``P x I`` matrix of the reference never exists, and one word is read back at the end.

    :param t: a :class:`Tensor` (Tucker factors are contracted in first; ``t`` is not modified)
    :param P: how many samples to draw (default: 1)
    :param seed: an int reproduces the reference's thresholds (``np.random.default_rng(seed)``, ``rng.random(P)`` once per mode,
        drawn on the host and uploaded once); ``None`` draws ``torch.rand((P, N), dtype=torch.float64, device=...)`` on the device

    :return: an int64 matrix ``[P, N]`` on ``t``'s device

    Raises ValueError for batched tensors, for ``P < 0`` or a non-integer ``P``, for a rank above ``ttr_sample_max_rank()`` on
    device tensors and for a zero or non-finite conditional total; NotImplementedError for CP cores.
    """
    from .automata import _cores3

    try:
        P = operator.index(P)
    except TypeError:
        raise ValueError("sample: P must be a non-negative integer, got {!r}".format(P)) from None
    if P < 0:
        raise ValueError("sample: P must be a non-negative integer, got {}".format(P))
    cores = _cores3(t, "sample")
    dev, N = cores[0].device, len(cores)
    if seed is None:
        U = torch.rand((P, N), dtype=torch.float64, device=dev)
    else:
        rng = np.random.default_rng(seed=seed)
        U = torch.from_numpy(np.stack([rng.random(P) for _ in range(N)], axis=1)).to(dev)
    return _sample_sweep(cores, U)

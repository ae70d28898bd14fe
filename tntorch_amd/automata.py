"""Tensors read as weighted automata: masks that accept strings by their weight, and the enumeration of what a mask accepts.

Mirror of ``tntorch/automata.py`` (``weight_mask`` 6-23, ``weight_one_hot`` 26-51, ``weight`` 54-71, ``length`` 74-81,
``accepted_inputs`` 84-128).  The constructors build the reference's cores.  ``accepted_inputs`` is a level-by-level expansion of
the frontier of productive prefixes (``ttr_accept_count`` / ``ttr_accept_expand`` on device tensors) instead
of the reference's recursion with one ``matmul`` per prefix.

Unlike the reference:
  - the constructors take ``dtype`` and ``device`` (default: fp32 on the CPU, what the reference builds);
  - a negative ``weight`` and an ``nsymbols`` of the wrong length raise ValueError (the reference asserts);
  - ``accepted_inputs`` returns its matrix on the tensor's device, counts paths in fp64 whatever the cores' dtype, and raises
    ValueError for a tensor that is not integer-valued and non-negative (the reference leaves rows of zeros or overwrites rows);
    CP cores raise NotImplementedError.
"""

import torch

from ._dispatch import ops_for
from .tensor import Tensor, _not_in_scope

__all__ = ["weight_mask", "weight_one_hot", "weight", "length", "accepted_inputs"]


def _nsymbols(N, nsymbols, what):
    if not hasattr(nsymbols, "__len__"):
        nsymbols = [nsymbols] * N
    if len(nsymbols) != N:
        raise ValueError("{}: nsymbols must be an int or one per dimension ({}), got {}".format(what, N, len(nsymbols)))
    return [int(s) for s in nsymbols]


def weight_mask(N, weight, nsymbols=2, dtype=None, device=None):
    """Accepts a string iff its number of 1's (the sum of its symbols) equals, or is in, ``weight`` (automata.py:6-23).

    :param N: number of dimensions
    :param weight: an integer (or list thereof): recognized weight(s)
    :param nsymbols: slices per core (default is 2), an int or one per dimension

    :return: a mask :class:`Tensor`
    """
    if not hasattr(weight, "__len__"):
        weight = [weight]
    weight = torch.as_tensor(weight).long().reshape(-1)
    if weight.numel() == 0 or int(weight.min()) < 0:
        raise ValueError("weight_mask: weight must be one or more non-negative integers, got {}".format(weight.tolist()))
    t = weight_one_hot(N, int(weight.max()) + 1, nsymbols, dtype=dtype, device=device)
    last = t.cores[-1]
    t.cores[-1] = torch.sum(last[:, :, weight.to(last.device)], dim=2, keepdim=True)
    return t


def weight_one_hot(N, r=None, nsymbols=2, dtype=None, device=None):
    """Given a string of weight k, produces the one-hot encoding of k: the last rank (``r``, default N + 1) is the encoding's
    length (automata.py:26-51).

    :return: a :class:`Tensor` whose last core keeps its rank ``r``
    """
    nsymbols = _nsymbols(N, nsymbols, "weight_one_hot")
    if r is None:
        r = N + 1
    eye = torch.eye(r, dtype=dtype, device=device)
    cores = []
    for n in range(N):
        core = torch.zeros([r, nsymbols[n], r], dtype=dtype, device=device)
        core[:, 0, :] = eye
        for s in range(1, nsymbols[n]):
            core[:, s, s:] = eye[:, :r - s] if s < r else 0
        cores.append(core)
    cores[0] = cores[0][0:1, :, :]
    return Tensor(cores)


def weight(N, nsymbols=2, dtype=None, device=None):
    """For any string, counts how many 1's it has: the sum of its symbols (automata.py:54-71).

    :return: a :class:`Tensor` of ranks 2
    """
    cores = []
    for n in range(N):
        core = torch.eye(2, dtype=dtype, device=device)[:, None, :].repeat(1, nsymbols, 1)
        core[1, :, 0] = torch.arange(nsymbols, dtype=core.dtype, device=device)
        cores.append(core)
    cores[0] = cores[0][1:2, :, :]
    cores[-1] = cores[-1][:, :, 0:1]
    return Tensor(cores)


def length(N):
    """automata.py:74-81: a todo of the reference."""
    raise NotImplementedError


def _cores3(t, what):
    if not isinstance(t, Tensor):
        raise ValueError("{}: expected a tntorch_amd.Tensor, got {}".format(what, type(t).__name__))
    if t.batch:
        raise ValueError("Batched tensors are not supported.")
    if any(c.dim() == 2 for c in t.cores):
        _not_in_scope("{} of CP cores".format(what))
    return [c[0].contiguous() for c in t._absorbed4()]


def _total(t, what="sum"):
    """Sum of all entries of ``t`` as an fp64 0-dim tensor on its device: the chain of right environments."""
    cores = _cores3(t, what)
    return ops_for(cores[0]).accept_fibers(cores)[1].sum()


def accepted_inputs(t):
    """All strings accepted by an automaton, in lexicographic order; string ``s`` appears ``t[s]`` times (automata.py:84-128).

    ``t`` must be integer-valued and non-negative.  The frontier of productive prefixes is expanded one mode at a time: the
    counts of a prefix's children are ``rint(L . core[:, i, :] . right)``, children with a count of zero are dropped before their
    left vector is computed, and every child writes its symbol into its run of output rows.  Paths are counted in fp64 (exact up
    to 2^53) whatever the cores' dtype.  Host reads: the number of rows, one frontier size per mode, and one consistency word.

    :param t: a :class:`Tensor` (Tucker factors are contracted in first)

    :return: an int64 matrix ``[round(sum t), N]`` on ``t``'s device, one string per row

    Raises ValueError for batched tensors, for a rank above ``ttr_accept_max_rank()`` on device tensors, and where the rounded
    counts of some prefix's children are negative or do not add up to the prefix's own count (``t`` is not integer-valued and
    non-negative); NotImplementedError for CP cores.  The check sees the counts of the prefixes that are expanded: entries that
    cancel inside a prefix whose count is zero are dropped with it.
    """
    cores = _cores3(t, "accepted_inputs")
    ops = ops_for(cores[0])
    dev, N = cores[0].device, len(cores)
    fibers, right0 = ops.accept_fibers(cores)
    S = int(torch.round(right0.sum()).item())
    if S < 0:
        raise ValueError("accepted_inputs: the tensor sums to {}: it must be integer-valued and non-negative".format(S))
    Xs = torch.empty((S, N), dtype=torch.int64, device=dev)
    if S == 0:
        return Xs
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    L = torch.ones((1, cores[0].shape[0]), dtype=torch.float64, device=dev)
    off = torch.zeros(1, dtype=torch.int64, device=dev)
    cnt = torch.full((1,), S, dtype=torch.int64, device=dev)
    for mu in range(N):
        C = ops.accept_count(L, fibers[mu])
        childoff = off[:, None] + (torch.cumsum(C, dim=1) - C)
        productive = C.reshape(-1) > 0
        K = int(productive.sum().item())
        idx = torch.nonzero_static(productive, size=K).reshape(-1)
        L, off, cnt = ops.accept_expand(L, cores[mu], C, childoff, cnt, idx, Xs, mu, flag, mu == N - 1)
        if K == 0:
            break
    word = int(flag.item())
    if word != 0:
        raise ValueError("accepted_inputs: the tensor must be integer-valued and non-negative (the rounded counts of a prefix's "
                         "children are negative or do not add up to the prefix's count; consistency word {})".format(word))
    return Xs

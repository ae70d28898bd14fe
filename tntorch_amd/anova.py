"""ANOVA decomposition and variance-based sensitivity (Sobol indices) on tensor trains.

Mirror of ``tntorch/anova.py`` (``anova_decomposition`` 9-43, ``undo_anova_decomposition`` 46-64, ``truncate_anova`` 67-96,
``sobol`` 99-148, ``mean_dimension`` 151-176, ``dimension_distribution`` 179-201).  ``anova_decomposition`` builds the reference's
extended TT-Tucker tensor (one extra slice per mode for "variable not selected"); ``sobol`` does NOT build it: it carries two
stacks of environments through the train, "no variable selected so far" and "at least one", and mixes them with the mask's
cores.  Every step is one centred, weighted sandwich ``sum_i w_i (A_i - mu)^T Z (A_i - mu)``
(``ttr_mode_sandwich`` on device tensors), so the empty tuple is excluded by never adding it: nothing is subtracted, and every
term is non-negative for a positive semi-definite interface.

Unlike the reference, in every function here:
  - everything follows the input's device and dtype, fp32 or fp64 (the reference builds fp32 CPU marginals and constants);
  - the marginals are normalised on a copy: a list passed in is never modified (the reference's ``sobol`` divides the caller's
    vectors in place);
  - batched tensors raise ValueError, CP cores NotImplementedError;
  - marginals of the wrong length or sizes, a mask with the wrong number of modes and an argument that is not a ``Tensor`` raise
    ValueError (the reference asserts, or fails in an einsum);
  - ``sobol`` computes the variance of the selected terms from environments instead of ``dot(a, mask(am, m)) / dot(a, am)`` on
    the extended train minus a rank-1 train (in fp32 that subtraction cancels whenever the mean dominates the variance).
"""

import numpy as np
import torch

from ._dispatch import ops_for
from .derivatives import _check_tensor, _cores3
from .tensor import Tensor

__all__ = ["anova_decomposition", "undo_anova_decomposition", "truncate_anova", "sobol", "mean_dimension", "dimension_distribution"]


# ---------------------------------------------------------------------------------------------- arguments
def _weights(t, marginals, what):
    """One weight vector [I_n] per mode on ``t``'s device, in its dtype: the marginal normalised to sum 1 on a copy; ``None`` (the
    whole list or one entry): uniform."""
    c0 = t.cores[0]
    shape = t.shape
    if marginals is None:
        marginals = [None] * len(shape)
    if not hasattr(marginals, "__len__") or len(marginals) != len(shape):
        raise ValueError("{}: marginals: expected one vector (or None) per mode ({}), got {!r}".format(
            what, len(shape), len(marginals) if hasattr(marginals, "__len__") else marginals))
    out = []
    for n, marg in enumerate(marginals):
        if marg is None:
            out.append(torch.full((shape[n],), 1.0 / shape[n], dtype=c0.dtype, device=c0.device))
            continue
        m = torch.as_tensor(marg).to(device=c0.device, dtype=c0.dtype)
        if m.dim() != 1 or m.shape[0] != shape[n]:
            raise ValueError("{}: marginals[{}]: expected a vector of {} entries, got shape {}".format(what, n, shape[n], tuple(m.shape)))
        out.append((m / m.sum()).contiguous())
    return out


def _check_mask(t, mask, what):
    _check_tensor(mask, what + " (mask)")
    if mask.dim() != t.dim():
        raise ValueError("{}: the tensor has {} modes, the mask {}".format(what, t.dim(), mask.dim()))


# ---------------------------------------------------------------------------------------------- the extended tensor
def anova_decomposition(t, marginals=None):
    """The extended tensor that contains all terms of the ANOVA decomposition of ``t`` (anova.py:9-43; Ballester-Ripoll, Paredes
    and Pajarola, "Sobol Tensor Trains for Global Sensitivity Analysis", 2017): mode ``n`` gets the Tucker factor
    ``[expected; U - expected]`` of ``I_n + 1`` rows (``U`` the mode's factor, or the identity; ``expected`` its mean under the
    marginal) and ``idxs[n] = [0] + [1] * I_n``: slice 0 integrates the variable out, slice ``1 + i`` is the centred slice ``i``.
    The cores are copies of ``t``'s.

    :param t: ND input :class:`Tensor`
    :param marginals: list of N vectors, the PMF of each variable (``None``, or ``None`` entries, for uniform distributions);
        normalised to sum 1 on a copy
    :return: a :class:`Tensor`
    """
    _check_tensor(t, "anova_decomposition")
    w = _weights(t, marginals, "anova_decomposition")
    c0 = t.cores[0]
    Us, idxs = [], []
    for n, I in enumerate(t.shape):
        U = torch.eye(I, dtype=c0.dtype, device=c0.device) if t.Us[n] is None else t.Us[n].to(c0.dtype)
        expected = torch.sum(U * w[n][:, None], dim=0, keepdim=True)
        Us.append(torch.cat((expected, U - expected), dim=0))
        idxs.append([0] + [1] * I)
    return Tensor([c.clone() for c in t.cores], Us=Us, idxs=idxs)


def undo_anova_decomposition(a):
    """Undo :func:`anova_decomposition` (anova.py:46-64): slice ``i`` of the result is slice 0 plus slice ``1 + i`` of ``a``, on
    the Tucker factor where the mode has one, else on the core.

    :param a: a :class:`Tensor` obtained with :func:`anova_decomposition`
    :return: a :class:`Tensor` that has ``a`` as its ANOVA tensor
    """
    _check_tensor(a, "undo_anova_decomposition")
    cores, Us = [], []
    for n in range(a.dim()):
        if a.Us[n] is None:
            cores.append(a.cores[n][..., 1:, :] + a.cores[n][..., 0:1, :])
            Us.append(None)
        else:
            cores.append(a.cores[n].clone())
            Us.append(a.Us[n][1:, :] + a.Us[n][0:1, :])
    return Tensor(cores, Us=Us)


def truncate_anova(t, mask, keepdim=False, marginals=None):
    """The function that is left of ``t`` after deleting all ANOVA terms that do not satisfy ``mask`` (anova.py:67-96):
    ``undo(mask(anova(t), mask))``; without ``keepdim`` the modes no accepted tuple of the mask selects are dropped (index 0 of a
    dummy mode; ``accepted_inputs`` decides).

    >>> x = tn.symbols(t.dim())[0]
    >>> t2 = tn.truncate_anova(t, mask=tn.only(x), keepdim=False)   # depends on one variable only

    :param t: an N-dimensional :class:`Tensor`
    :param mask: an N-dimensional mask
    :param keepdim: if True, all dummy dimensions are preserved.  Default is False
    :param marginals: see :func:`anova_decomposition`.  Defaults to uniform marginals
    :return: a :class:`Tensor`
    """
    from .automata import accepted_inputs
    from .tools import mask as apply_mask

    _check_tensor(t, "truncate_anova")
    _check_mask(t, mask, "truncate_anova")
    out = undo_anova_decomposition(apply_mask(anova_decomposition(t, marginals=marginals), mask))
    if not keepdim:
        affecting = accepted_inputs(mask).sum(dim=0).cpu().numpy()
        slices = [0] * t.dim()
        for i in np.where(affecting)[0]:
            slices[int(i)] = slice(None)
        out = out[tuple(slices)]
    return out


# ---------------------------------------------------------------------------------------------- Sobol indices
def _mask_slices(mask, c0):
    """Per mode the mask's matrices (M[:, 0, :], M[:, 1, :]) on ``c0``'s device, in its dtype: Tucker factor contracted in, slice
    index clamped to the mask's size as ``tn.mask`` does (slice 0: variable not selected, slice 1: selected)."""
    out = []
    for core in _cores3(mask, "sobol (mask)"):
        core = core.to(device=c0.device, dtype=c0.dtype)
        out.append((core[:, 0, :], core[:, min(1, core.shape[1] - 1), :]))
    return out


def _block_diag_one(M):
    """[[M, 0], [0, 1]]: the all-ones mask of the denominator rides along as one more boundary rank."""
    S, Sn = M.shape
    out = M.new_zeros((S + 1, Sn + 1))
    out[:S, :Sn] = M
    out[S, Sn] = 1
    return out


def _selected_variance(t, mask, marginals, with_total, what):
    """The variance of the ANOVA terms ``mask`` accepts, the empty tuple excluded: one value per trailing rank of the mask (a
    vector [S_N]); with ``with_total`` one more entry, the same for the mask that accepts everything (the total variance).

    With mu = sum_i w_i A_i, P(Z)[s] = mu^T Z[s] mu (variable integrated out) and Q(Z)[s] = sum_i w_i (A_i - mu)^T Z[s] (A_i - mu)
    (variable selected) and the mix mix_b(X)[s'] = sum_s M[s, b, s'] X[s], the environments of "nothing selected so far" (Z0)
    and "something selected" (Z1) move through mode n as
        Z0' = mix_0(P(Z0)),    Z1' = mix_1(Q(Z0)) + mix_0(P(Z1)) + mix_1(Q(Z1)),
    from Z0 = ones, Z1 = 0.  Z0 and Z1 are stacked: one P launch, one Q launch and one small GEMM (the mix) per mode."""
    A = _cores3(t, what)
    _check_mask(t, mask, what)
    w = _weights(t, marginals, what)
    ops = ops_for(A[0])
    Ms = _mask_slices(mask, A[0])
    if with_total:
        Ms = [(_block_diag_one(M0), _block_diag_one(M1)) for M0, M1 in Ms]
    S, R = Ms[0][0].shape[0], A[0].shape[0]
    Z = torch.cat([A[0].new_ones((S, R, R)), A[0].new_zeros((S, R, R))])   # [Z0; Z1]
    for n, core in enumerate(A):
        C = core.shape[2]
        mu = ops.mode_reduce(core, w[n])
        P = ops.mode_sandwich(Z, mu[:, None, :].contiguous(), None, None)
        Q = ops.mode_sandwich(Z, core, w[n], mu)
        M0t, M1t = Ms[n][0].t(), Ms[n][1].t()
        zero = torch.zeros_like(M0t)
        mix = torch.cat([torch.cat([M0t, zero, zero, zero], dim=1), torch.cat([zero, M0t, M1t, M1t], dim=1)])   # [2 S', 4 S]
        X = torch.cat([P, Q]).reshape(1, 4 * S, C * C)   # rows: P(Z0), P(Z1), Q(Z0), Q(Z1)
        S = M0t.shape[0]
        Z = ops.mm(mix[None].contiguous(), X).reshape(2 * S, C, C)
    return ops.mode_reduce(Z[S:].reshape(S, -1, 1).contiguous()).reshape(S)


def sobol(t, mask, marginals=None, normalize=True):
    """Sobol indices (as given by a certain mask) of a tensor with independently distributed input variables (anova.py:99-148;
    Ballester-Ripoll, Paredes and Pajarola, 2017): the variance of the ANOVA terms the mask accepts over the total variance.

    :param t: an N-dimensional :class:`Tensor`
    :param mask: an N-dimensional mask
    :param marginals: a list of N vectors (normalised to sum 1 on a copy).  If None (default), uniform distributions are assumed
    :param normalize: whether to divide by the total variance of the model (True by default)
    :return: a 0-dim tensor >= 0 on ``t``'s device, in its dtype; for a mask whose last rank is above 1 (``weight_one_hot``) a
        one-mode :class:`Tensor` of that length.  A leading rank above 1, of ``t`` or of the mask, is summed away

    Unlike the reference: computed from environments, no extended train, no masked train and no subtraction (module docstring);
    the marginals are not modified.
    """
    v = _selected_variance(t, mask, marginals, bool(normalize), "sobol")
    if normalize:
        v = v[:-1] / v[-1]
    if v.shape[0] == 1:
        return v.reshape(())
    return Tensor([v.reshape(1, -1, 1)])


def mean_dimension(t, mask=None, marginals=None):
    """The mean dimension of ``t`` under the given marginals (anova.py:151-176; Caflisch, Morokoff and Owen, 1997): 1 for a purely
    additive function.  With ``mask``: restricted to the terms the mask accepts.

    :return: a 0-dim tensor >= 1
    """
    from .automata import weight
    from .tools import mask as apply_mask

    _check_tensor(t, "mean_dimension")
    c0 = t.cores[0]
    wt = weight(t.dim(), dtype=c0.dtype, device=c0.device)
    if mask is None:
        return sobol(t, wt, marginals=marginals)
    _check_mask(t, mask, "mean_dimension")
    return sobol(t, apply_mask(wt, mask), marginals=marginals) / sobol(t, mask, marginals=marginals)


def dimension_distribution(t, mask=None, order=None, marginals=None):
    """The dimension distribution of ``t`` (anova.py:179-201): entry ``k - 1`` is the share of the variance carried by the ANOVA
    terms of order ``k``.

    :param mask: an optional mask :class:`Tensor` to restrict to
    :param order: int, compute only this many order contributions.  By default, all N are returned
    :return: a vector of ``order`` entries on ``t``'s device, in its dtype
    """
    from .automata import weight_one_hot
    from .tools import mask as apply_mask

    _check_tensor(t, "dimension_distribution")
    if order is None:
        order = t.dim()
    if int(order) != order or order < 1:
        raise ValueError("dimension_distribution: order must be an integer >= 1, got {!r}".format(order))
    c0 = t.cores[0]
    oh = weight_one_hot(t.dim(), int(order) + 1, dtype=c0.dtype, device=c0.device)
    if mask is None:
        return sobol(t, oh, marginals=marginals).torch()[1:]
    _check_mask(t, mask, "dimension_distribution")
    return sobol(t, apply_mask(oh, mask), marginals=marginals).torch()[1:] / sobol(t, mask, marginals=marginals)

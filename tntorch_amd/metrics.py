"""Inner products / error metrics on tensor trains used by the parity tests.

Mirror of the TT subset of ``tntorch/metrics.py`` (``dot`` 28-116, ``dist`` 119-132,
``relative_error`` 135-151, ``normsq`` 457-466, ``norm`` 469-478): the consumers of the hot path
(SURVEY 8f-4).  The contraction runs on the HIP GEMM for device tensors and on torch for CPU tensors.

The moment family (``hadamard_sum`` 345-455, ``raw_moment`` 303-319, ``normalized_moment`` 322-342, ``var`` 247-263, ``std``
266-275) sits on the rounding sweeps and two contractions of its own (``ttr_core_matvec``, ``ttr_hsum_step``).
"""

import torch

from ._dispatch import ops_for
from .tensor import Tensor

__all__ = ["dot", "dist", "relative_error", "normsq", "norm", "hadamard_sum", "raw_moment", "normalized_moment", "var", "std"]


def _dense(t):
    return t.torch() if isinstance(t, Tensor) else t


def dot(t1, t2):
    """Full inner product <t1, t2> (metrics.py:28-116 with k = N, no Tucker factors)."""
    if not isinstance(t1, Tensor) or not isinstance(t2, Tensor):
        a, b = _dense(t1), _dense(t2)
        ops_for(b)  # (refuses a device operand that requires grad: dense_dot has no backward)
        return ops_for(a).dense_dot(a, b)
    if t1.batch or t2.batch:
        raise ValueError("Batched tensors are not supproted.")
    if t1.shape != t2.shape:
        raise ValueError("Dot product requires leading dimensions to be equal, but they are {} and {}".format(t1.shape, t2.shape))
    c1 = t1._absorbed4()  # Tucker factors contracted in (the reference contracts U1^T U2 instead: same value)
    return ops_for(c1[0]).dot(c1, t2._absorbed4())  # device tensors: Lprod chain on ttr_gemm


def dist(t1, t2):
    """Euclidean distance (metrics.py:119-132)."""
    if not isinstance(t1, Tensor) or not isinstance(t2, Tensor):
        a, b = _dense(t1), _dense(t2)
        return ops_for(a, grad=True).dense_dist(a, b)  # differentiable in both operands on the device (autodiff.dense_dist)
    return torch.sqrt((dot(t1, t1) + dot(t2, t2) - 2 * dot(t1, t2)).clamp(0))


def relative_error(gt, approx):
    """||gt - approx|| / ||gt|| (metrics.py:135-151).

    Between two compressed tensors this uses the reference's <a,a>+<b,b>-2<a,b> formula and
    is therefore limited to ~sqrt(machine eps) by cancellation.
    """
    if not isinstance(gt, Tensor) or not isinstance(approx, Tensor):
        a, b = _dense(gt), _dense(approx)
        ops = ops_for(a)  # (gt itself may not require grad on the device: dense_norm has no backward)
        return ops.dense_dist(a, b) / ops.dense_norm(a)  # differentiable in ``approx`` (autodiff.dense_dist)
    dotgt = dot(gt, gt)
    return torch.sqrt((dotgt + dot(approx, approx) - 2 * dot(gt, approx)).clamp(0)) / torch.sqrt(dotgt.clamp(0))


def normsq(t):
    return dot(t, t)


def norm(t):
    return torch.sqrt(torch.clamp(normsq(t), min=0))


# ---------------------------------------------------------------------------------------------- moments (metrics.py:247-455)
def _tt_cores3(t, what):
    """The cores [r, I, r'] of a non-batch TT tensor with its Tucker factors contracted in; the refusals of ``dot`` / indexing."""
    from .tensor import _not_in_scope

    if not isinstance(t, Tensor):
        raise ValueError("{}: expected a tntorch_amd.Tensor, got {}".format(what, type(t).__name__))
    if t.batch:
        raise ValueError("Batched tensors are not supported.")
    if any(c.dim() == 2 for c in t.cores):
        _not_in_scope("{} of CP cores".format(what))
    return [c[0] for c in t._absorbed4()]


def _pdf(t, marginals):
    """Rank-1 train of the marginals, each normalised to sum 1 on a copy (``None``: the uniform weights 1 / I_n)."""
    c0 = t.cores[0]
    shape = t.shape
    if marginals is None:
        return Tensor([torch.full((1, I, 1), 1.0 / I, dtype=c0.dtype, device=c0.device) for I in shape])
    if len(marginals) != len(shape):
        raise ValueError("marginals: expected one vector per mode ({}), got {}".format(len(shape), len(marginals)))
    cores = []
    for n, marg in enumerate(marginals):
        m = torch.as_tensor(marg).to(device=c0.device, dtype=c0.dtype)
        if m.dim() != 1 or m.shape[0] != shape[n]:
            raise ValueError("marginals[{}]: expected a vector of {} entries, got shape {}".format(n, shape[n], tuple(m.shape)))
        cores.append((m / m.sum())[None, :, None])
    return Tensor(cores)


def _mean(t, pdf):
    return dot(t, pdf)


def _centered(t, mean):
    """t - mean for a 0-dim ``mean`` that stays on its device (no host read)."""
    c0 = t.cores[0]
    cores = [torch.ones((1, I, 1), dtype=c0.dtype, device=c0.device) for I in t.shape]
    cores[0] = cores[0] * (-mean)
    return t + Tensor(cores)


def _hsum_exact(ops, cs):
    """metrics.py:407-425: cs[m][n] = core n of tensor m; one ``hsum_step`` per mode on the running K-way interface."""
    W = torch.ones([c[0].shape[0] for c in cs], dtype=cs[0][0].dtype, device=cs[0][0].device)
    for n in range(len(cs[0])):
        W = ops.hsum_step(W, [c[n] for c in cs])
    return (ops.sum_all(W) if W.numel() > 1 else W).reshape(())


def _hsum_approx(ops, cs, eps, algorithm):
    """metrics.py:427-454: per mode, the rounded train of diagonal cores (a TT-matrix over the rank pairs) is applied to the
    running TT-vector (``core_matvec``) and the product is rounded again."""
    M, N = len(cs), len(cs[0])

    def mode_matrix(n):
        D = ops.diag_cores([c[n] for c in cs])
        if M > 1:
            D = ops.round_tt(D, eps, [None] * (M - 1), algorithm, False)
        return [D[m][0].reshape(D[m].shape[1], cs[m][n].shape[0], cs[m][n].shape[2], D[m].shape[3]) for m in range(M)]

    G = mode_matrix(0)
    if all(g.shape[1] == 1 for g in G):
        x = [g.reshape(g.shape[0], g.shape[2], g.shape[3]) for g in G]
    else:  # a boundary rank above 1 is summed away, as ``dot`` does
        x = [ops.core_matvec(g.new_ones((1, g.shape[1], 1)), g) for g in G]
    for n in range(1, N):
        G = mode_matrix(n)
        x = [ops.core_matvec(x[m], G[m])[None] for m in range(M)]
        if M > 1:
            x = ops.round_tt(x, eps, [None] * (M - 1), algorithm, False)
        x = [c[0] for c in x]
    out = ops.decompress([c[None] for c in x])   # [1, r_1, .., r_M] over the trailing boundary ranks (all 1 as a rule): a GEMM chain
    return (ops.sum_all(out) if out.numel() > 1 else out).reshape(())


def hadamard_sum(ts, algorithm="exact", eps=None):
    """Sum of the element-wise product t_1 o ... o t_M of tensors of equal shape (metrics.py:345-455).

    ``algorithm``: ``"exact"`` (default) contracts the M trains mode by mode (one ``ttr_hsum_step`` per mode on device tensors: the
    interface has prod_m r_m entries); ``"eig"`` / ``"svd"`` is the approximate algorithm of the reference, a variant of Novikov
    et al., "Putting MRFs on a Tensor Train" (2014), Alg. 1, with relative error ``eps`` in each of its two roundings per mode.

    Unlike the reference, everything follows the inputs' device and dtype (fp32 or fp64; the reference builds fp32 CPU
    intermediates: fp64 fails in ``"exact"`` and is squeezed through fp32 otherwise); the result is a 0-dim tensor on that device,
    as ``tn.dot`` returns here, with no host synchronisation; Tucker factors are contracted into the cores first; CP cores are
    out of scope (NotImplementedError) and batched tensors a ValueError, as for ``tn.dot`` and indexing; unequal shapes, an
    unknown algorithm, or ``eps=None`` with an approximate algorithm raise ValueError (the reference asserts, or fails inside
    the rounding); a one-mode tensor returns its value (the reference's approximate path returns None); boundary ranks above 1
    are summed away, as ``tn.dot`` does here.  With device tensors the exact algorithm raises ValueError when prod_m r_m makes
    its scratch exceed what ``ttr_hsum_step`` accepts: use ``algorithm="eig"`` then.
    """
    ts = list(ts)
    if len(ts) < 1:
        raise ValueError("hadamard_sum: at least one tensor is needed")
    if algorithm not in ("exact", "eig", "svd"):
        raise ValueError('hadamard_sum: algorithm must be "exact", "eig" or "svd", got {!r}'.format(algorithm))
    if algorithm != "exact" and eps is None:
        raise ValueError('hadamard_sum: algorithm="{}" needs eps (the relative error of each rounding step)'.format(algorithm))
    cs = [_tt_cores3(t, "hadamard_sum") for t in ts]
    for t in ts[1:]:
        if t.shape != ts[0].shape:
            raise ValueError("hadamard_sum: all tensors must have the same shape, got {} and {}".format(ts[0].shape, t.shape))
    c0 = cs[0][0]
    if any(c.dtype != c0.dtype or c.device != c0.device for tc in cs for c in tc):
        raise ValueError("hadamard_sum: all tensors must share one dtype and one device")
    ops = ops_for(c0)
    if algorithm == "exact":
        return _hsum_exact(ops, cs)
    return _hsum_approx(ops, cs, eps, algorithm)


def _check_order(k):
    if int(k) != k or k < 1:
        raise ValueError("the moment order k must be an integer >= 1, got {!r}".format(k))
    return int(k)


def raw_moment(t, k, marginals=None, eps=1e-6, algorithm="eig"):
    """k-th raw moment E[t^k] (metrics.py:303-319): ``hadamard_sum`` of k copies of ``t``, the last one weighted by the
    marginals' product density, or divided by the number of entries when ``marginals`` is None.

    Unlike the reference: device, dtype, result and refusals as for ``hadamard_sum``; ``k < 1`` and marginals of the wrong
    length or sizes raise ValueError; the marginals are normalised on a copy, never in place.
    """
    k = _check_order(k)
    _tt_cores3(t, "raw_moment")
    if marginals is not None:
        return hadamard_sum([t] * (k - 1) + [t * _pdf(t, marginals)], eps=eps, algorithm=algorithm)
    return hadamard_sum([t] * k, eps=eps, algorithm=algorithm) / float(t.numel())


def var(t, marginals=None):
    """Variance of the entries of ``t`` (metrics.py:247-263), optionally under a product density of ``marginals``.  The mean is
    an inner product with a rank-1 train.  Unlike the reference: see ``raw_moment``."""
    _tt_cores3(t, "var")
    pdf = _pdf(t, marginals)
    tc = _centered(t, _mean(t, pdf))
    if marginals is not None:
        return dot(tc * pdf, tc)
    return normsq(tc) / float(t.numel())


def std(t):
    """Standard deviation of the entries of ``t`` (metrics.py:266-275): sqrt(max(var, 0)), a 0-dim tensor on ``t``'s device."""
    return torch.sqrt(torch.clamp(var(t), min=0))


def normalized_moment(t, k, marginals=None, eps=1e-12, algorithm="eig"):
    """k-th normalized central moment E[(t - E[t])^k] / sigma^k (metrics.py:322-342).  Unlike the reference: see ``raw_moment``."""
    k = _check_order(k)
    _tt_cores3(t, "normalized_moment")
    tc = _centered(t, _mean(t, _pdf(t, marginals)))
    return raw_moment(tc, k, marginals=marginals, eps=eps, algorithm=algorithm) / var(t, marginals=marginals) ** (k / 2.0)

"""Differential operators and derivative-based sensitivity on tensor trains.

Mirror of ``tntorch/derivatives.py`` (``partial`` 72-130, ``gradient`` 133-157, ``active_subspace`` 160-201, ``dgsm`` 204-235,
``divergence`` 238-258, ``curl`` 261-283, ``laplacian`` 286-302).  A derivative is a stencil on ONE core (``ttr_mode_diff``);
``laplacian`` builds the exact rank-2r train of the sum of one-site operators (``ttr_laplace_core``) instead of adding N trains;
``dgsm`` / ``active_subspace`` contract left and right environments with ``ttr_hsum_step`` instead of building N gradient trains
and N (N + 1) / 2 product trains.  ``partialset`` (6-69) stacks the forward differences of every mode
behind the mode itself and selects the partials of the wanted orders with ``automata.weight_mask`` and ``tools.mask``.

Unlike the reference, in every function here:
  - everything follows the input's device and dtype, fp32 or fp64 (the reference puts the ``dgsm`` / ``active_subspace`` results
    and its default marginals in fp32 on the CPU);
  - the default bounds of mode ``d`` are ``[0, t.shape[d]]`` of THAT mode (the reference indexes its default bounds by the
    position in ``dim``, so ``partial(t, 2)`` takes mode 0's extent, and ``laplacian`` / ``divergence`` without bounds take
    mode 0's extent for every mode);
  - batched tensors raise ValueError, CP cores NotImplementedError;
  - wrong lengths of ``bounds`` / ``marginals`` / ``ts``, unequal shapes, ``order < 1``, a ``dim`` out of range and a ``curl`` of
    anything but three 3-mode tensors raise ValueError (the reference asserts, or fails further down);
  - ``partialset`` divides every difference of mode ``n`` by the same step ``(b1 - b0) / (t.shape[n] - 1)`` (the reference
    recomputes the step from the shrinking stack, so with default bounds its second difference no longer has step 1).
"""

import torch

from ._dispatch import ops_for
from .tensor import Tensor, _not_in_scope

__all__ = ["partialset", "partial", "gradient", "divergence", "curl", "laplacian", "dgsm", "active_subspace"]


# ---------------------------------------------------------------------------------------------- arguments
def _check_tensor(t, what):
    if not isinstance(t, Tensor):
        raise ValueError("{}: expected a tntorch_amd.Tensor, got {}".format(what, type(t).__name__))
    if t.batch:
        raise ValueError("Batched tensors are not supported.")
    if any(c.dim() == 2 for c in t.cores):
        _not_in_scope("{} of CP cores".format(what))


def _cores3(t, what):
    """Contiguous cores [r, I, r'] with the Tucker factors contracted in."""
    _check_tensor(t, what)
    return [c[0].contiguous() for c in t._absorbed4()]


def _is_pair(b):
    return hasattr(b, "__len__") and len(b) == 2 and not hasattr(b[0], "__len__") and not hasattr(b[1], "__len__")


def _mode_bounds(t, dims, bounds, what):
    """One (b0, b1) per entry of ``dims``: ``None`` -> [0, t.shape[d]] of that mode; one pair -> that pair for every mode;
    otherwise one pair per entry of ``dims``."""
    shape = t.shape
    if bounds is None:
        out = [(0.0, float(shape[d])) for d in dims]
    elif _is_pair(bounds):
        out = [(float(bounds[0]), float(bounds[1]))] * len(dims)
    else:
        if not hasattr(bounds, "__len__") or len(bounds) != len(dims):
            raise ValueError("{}: bounds must be one pair [b0, b1] or one pair per mode ({}), got {!r}".format(what, len(dims), bounds))
        out = []
        for d, b in zip(dims, bounds):
            if b is None:
                out.append((0.0, float(shape[d])))
            elif _is_pair(b):
                out.append((float(b[0]), float(b[1])))
            else:
                raise ValueError("{}: bounds[{}] must be a pair [b0, b1], got {!r}".format(what, len(out), b))
    for b0, b1 in out:
        if b1 == b0:
            raise ValueError("{}: empty range [{}, {}] in bounds".format(what, b0, b1))
    return out


def _inv_step(I, b):
    """1 / step of derivatives.py:96: step = (b1 - b0) / (I + 1) * 2."""
    return (I + 1) / (2.0 * (b[1] - b[0]))


def _dims(t, dim, what):
    dims = list(dim) if hasattr(dim, "__len__") or isinstance(dim, range) else [dim]
    N = t.dim()
    out = []
    for d in dims:
        if int(d) != d or not -N <= d < N:
            raise ValueError("{}: dim {!r} out of range for a tensor of {} modes".format(what, d, N))
        out.append(int(d) % N)
    return out


# ---------------------------------------------------------------------------------------------- partialset
def partialset(t, order=1, mask=None, bounds=None):
    """A tensor that holds all partial derivatives of certain order(s), optionally restricted by a mask (derivatives.py:6-69).
    No padding: mode ``n`` of the result is the mode itself followed by its forward differences of order 1 .. max(order), of
    sizes I, I - 1, ..., and ``result.idxs[n]`` gives the order of every slice.  An entry whose slices have orders
    (o_1, .., o_N) is that mixed forward difference of ``t`` where ``sum o_n`` is in ``order`` (and ``mask`` accepts the modes
    with ``o_n > 0``), and zero elsewhere.

    >>> x, y, z = tn.symbols(3)
    >>> tn.partialset(t, 1, x)                 # x
    >>> tn.partialset(t, 2, x)                 # xx, xy, xz
    >>> tn.partialset(t, 2, tn.only(y | z))    # yy, yz, zz

    :param order: an int or list of ints.  Default is 1
    :param mask: an optional 2^N mask :class:`Tensor` to select only a subset of partials
    :param bounds: one pair [b0, b1] per mode; every difference of mode ``n`` is divided by the step ``(b1 - b0) / (I_n - 1)``.
        Default: ``[0, I_n - 1]``, all steps 1

    Unlike the reference: the step of a mode is the same for every order (see the module docstring); a mode too short for
    ``max(order)`` differences (a mode of size 1 for any order) and batched tensors raise ValueError.
    """
    from .automata import weight_mask
    from .tools import mask as apply_mask

    cores = _cores3(t, "partialset")
    N = len(cores)
    orders = [int(o) for o in order] if hasattr(order, "__len__") else [int(order)]
    if not orders or min(orders) < 0:
        raise ValueError("partialset: order must be one or more non-negative integers, got {!r}".format(order))
    max_order = max(orders)
    if bounds is None:
        bounds = [[0, c.shape[1] - 1] for c in cores]
    if len(bounds) != N or not all(_is_pair(b) for b in bounds):
        raise ValueError("partialset: bounds must be one pair [b0, b1] per mode ({}), got {!r}".format(N, bounds))
    stacked, idxs = [], []
    for n, core in enumerate(cores):
        I = core.shape[1]
        if I < 2 or I < max_order + 1:
            raise ValueError("Tensor size {} along dimension {} not enough to compute high-order derivative".format(I, n))
        if bounds[n][1] == bounds[n][0]:
            raise ValueError("partialset: empty range {!r} in bounds".format(list(bounds[n])))
        inv_step = (I - 1) / float(bounds[n][1] - bounds[n][0])
        stack = [core]
        for o in range(max_order):
            stack.append((stack[-1][:, 1:, :] - stack[-1][:, :-1, :]) * inv_step)
        stacked.append(torch.cat(stack, dim=1))
        idxs.append(torch.cat([torch.full((s.shape[1],), o, dtype=torch.int64, device=core.device) for o, s in enumerate(stack)]))
    d = Tensor(stacked, idxs=idxs)
    wm = weight_mask(N, orders, nsymbols=max_order + 1, dtype=cores[0].dtype, device=cores[0].device)
    if mask is not None:
        wm = apply_mask(wm, mask)
    result = apply_mask(d, wm)
    result.idxs = idxs
    return result


# ---------------------------------------------------------------------------------------------- partial / gradient
def partial(t, dim, order=1, bounds=None, periodic=False):
    """``order``-th partial derivative along ``dim`` (an int or a list of ints), derivatives.py:72-130: every pass multiplies the
    mode by ``S / step``, ``step = (b1 - b0) / (I + 1) * 2``, S the central-difference matrix with the reference's linearly
    extrapolated edge rows (or ``roll(-1) - roll(+1)`` where ``periodic``).  A mode with a Tucker factor is differentiated on the
    factor, the core is left alone.  ``bounds``: a pair (one ``dim``) or one pair per entry of ``dim``; ``periodic``: a bool or
    one per entry of ``dim``.  On device tensors: one ``ttr_mode_diff`` launch per mode for orders up to 4.

    Unlike the reference: see the module docstring (default bounds are those of the mode that is differentiated).
    """
    _check_tensor(t, "partial")
    dims = _dims(t, dim, "partial")
    if int(order) != order or order < 1:
        raise ValueError("partial: order must be an integer >= 1, got {!r}".format(order))
    bs = _mode_bounds(t, dims, bounds, "partial")
    pers = list(periodic) if hasattr(periodic, "__len__") else [periodic] * len(dims)
    if len(pers) != len(dims):
        raise ValueError("partial: periodic must be a bool or one per entry of dim ({}), got {}".format(len(dims), len(pers)))
    cores, Us = list(t.cores), list(t.Us)
    touched = set()
    shape = t.shape
    for d, b, per in zip(dims, bs, pers):
        inv = _inv_step(shape[d], b)
        if Us[d] is None:
            cores[d] = ops_for(cores[d]).mode_diff(cores[d], int(order), bool(per), inv)
        else:
            Us[d] = ops_for(Us[d]).mode_diff(Us[d][None], int(order), bool(per), inv)[0]
        touched.add(d)
    for n in range(t.dim()):  # the result shares nothing with its input (the reference clones the tensor first)
        if n not in touched or t.Us[n] is not None:
            cores[n] = t.cores[n].clone()
        if Us[n] is not None and n not in touched:
            Us[n] = Us[n].clone()
    return Tensor(cores, Us=Us, idxs=t._idxs)


def gradient(t, dim="all", bounds=None):
    """Gradient (derivatives.py:133-157): a list of ``partial(t, d, bounds=b)`` over ``dim`` (default: every mode), or one tensor
    when ``dim`` is an int.  ``bounds``: one pair for every mode, or one pair per entry of ``dim``.

    Unlike the reference: ``gradient(t, dim=int, bounds=...)`` passes the bounds as bounds (the reference passes them
    positionally as ``order``); otherwise see the module docstring.
    """
    _check_tensor(t, "gradient")
    if isinstance(dim, str):
        if dim != "all":
            raise ValueError('gradient: dim must be "all", an int or a list of ints, got {!r}'.format(dim))
        dim = list(range(t.dim()))
    single = not hasattr(dim, "__len__")
    dims = _dims(t, dim, "gradient")
    bs = _mode_bounds(t, dims, bounds, "gradient")
    out = [partial(t, d, order=1, bounds=list(b)) for d, b in zip(dims, bs)]
    return out[0] if single else out


# ---------------------------------------------------------------------------------------------- divergence / curl / laplacian
def _field(ts, what):
    ts = list(ts)
    for u in ts:
        _check_tensor(u, what)
    return ts


def divergence(ts, bounds=None):
    """Divergence of an N-mode vector field given as N tensors (derivatives.py:238-258): sum_n partial(ts[n], n), added with the
    trains' ``+`` (ranks add; round the result).  Unlike the reference: the sum does not start from a constant train; default
    bounds are per mode; a wrong number of tensors / bounds and unequal shapes raise ValueError."""
    ts = _field(ts, "divergence")
    if len(ts) < 1 or any(u.dim() != len(ts) for u in ts):
        raise ValueError("divergence: expected N tensors of N modes each, got {} tensors of {} modes".format(len(ts), [u.dim() for u in ts]))
    if any(u.shape != ts[0].shape for u in ts[1:]):
        raise ValueError("divergence: all tensors must have the same shape, got {}".format([tuple(u.shape) for u in ts]))
    bs = _mode_bounds(ts[0], list(range(len(ts))), bounds, "divergence")
    out = partial(ts[0], 0, bounds=list(bs[0]))
    for n in range(1, len(ts)):
        out = out + partial(ts[n], n, bounds=list(bs[n]))
    return out


def curl(ts, bounds=None):
    """Curl of a 3-mode vector field given as three tensors (derivatives.py:261-283); three tensors of the same shape.  Unlike the
    reference: anything but three 3-mode tensors of one shape raises ValueError (its first assert is always true)."""
    ts = _field(ts, "curl")
    if len(ts) != 3 or any(u.dim() != 3 for u in ts):
        raise ValueError("curl: expected three 3-mode tensors, got {} tensors of {} modes".format(len(ts), [u.dim() for u in ts]))
    if any(u.shape != ts[0].shape for u in ts[1:]):
        raise ValueError("curl: all tensors must have the same shape, got {}".format([tuple(u.shape) for u in ts]))
    b = [list(x) for x in _mode_bounds(ts[0], [0, 1, 2], bounds, "curl")]
    return [
        partial(ts[2], 1, bounds=b[1]) - partial(ts[1], 2, bounds=b[2]),
        partial(ts[0], 2, bounds=b[2]) - partial(ts[2], 0, bounds=b[0]),
        partial(ts[1], 0, bounds=b[0]) - partial(ts[0], 1, bounds=b[1]),
    ]


def laplacian(t, bounds=None):
    """Laplacian sum_n partial(t, n, order=2) (derivatives.py:286-302) as ONE train of ranks 2 r: with D_n = (S_n / step_n)^2 A_n
    the cores are [A_1 D_1], [[A_n, D_n], [0, A_n]], [D_N ; A_N] (one ``ttr_laplace_core`` launch per mode on device tensors); a
    one-mode tensor returns D_1.  Tucker factors are contracted in first: the result is a plain TT.

    Unlike the reference: ranks 2 r instead of N r + 1 (it adds N cloned trains to a constant one) -- the same tensor, and the
    rounding that follows costs the cube of the rank; default bounds are per mode; a wrong number of bounds raises ValueError.
    """
    cs = _cores3(t, "laplacian")
    N = len(cs)
    bs = _mode_bounds(t, list(range(N)), bounds, "laplacian")
    ops = ops_for(cs[0])
    invs = [_inv_step(c.shape[1], b) for c, b in zip(cs, bs)]
    if N == 1:
        return Tensor([ops.mode_diff(cs[0], 2, False, invs[0])])
    return Tensor([ops.laplace_core(c, 0 if n == 0 else (2 if n == N - 1 else 1), False, invs[n]) for n, c in enumerate(cs)])


# ---------------------------------------------------------------------------------------------- dgsm / active_subspace
def _weights(t, marginals, midpoint, what):
    """One weight core [1, I, 1] per mode: the marginal normalised to sum 1 on a copy (``None``: uniform), or, with ``midpoint``,
    the reference's (m[:-1] + m[1:]) / 2, normalised, with a trailing zero (derivatives.py:181-185)."""
    c0 = t.cores[0]
    shape = t.shape
    if marginals is None:
        marginals = [torch.full((I,), 1.0 / I, dtype=c0.dtype, device=c0.device) for I in shape]
    if len(marginals) != len(shape):
        raise ValueError("{}: marginals: expected one vector per mode ({}), got {}".format(what, len(shape), len(marginals)))
    cores = []
    for n, marg in enumerate(marginals):
        m = torch.as_tensor(marg).to(device=c0.device, dtype=c0.dtype)
        if m.dim() != 1 or m.shape[0] != shape[n]:
            raise ValueError("{}: marginals[{}]: expected a vector of {} entries, got shape {}".format(what, n, shape[n], tuple(m.shape)))
        if midpoint:
            m = (m[:-1] + m[1:]) / 2
            m = torch.cat([m / m.sum(), m.new_zeros(1)])
        else:
            m = m / m.sum()
        cores.append(m[None, :, None].contiguous())
    return cores


def _sensitivity(t, bounds, marginals, midpoint, full, what):
    """The entries <g_i * pdf, g_j> (g_n = partial(t, n), pdf the product of the weights) by the environment recursion: with
    D_n = diff(A_n), left environments L_n and right environments R_n of the weighted A-A transfer, the diagonal entry i is a D-D
    step on L_i closed with R_{i+1}; with ``full``, a D-A step on L_i starts a running interface that A-A steps carry on and an
    A-D step closed with R_{j+1} turns into entry (i, j) at every j > i.  Every step is one ``hsum_step`` with K = 3: core, weight
    vector as a [1, I, 1] core, core -- no weighted copy of a core is made.  Returns {(i, j): 0-dim tensor}, i <= j."""
    A = _cores3(t, what)
    N = len(A)
    bs = _mode_bounds(t, list(range(N)), bounds, what)
    w = _weights(t, marginals, midpoint, what)
    ops = ops_for(A[0])
    D = [ops.mode_diff(A[n], 1, False, _inv_step(A[n].shape[1], bs[n])) for n in range(N)]

    def step(W, X, n, Y):
        return ops.hsum_step(W, [X, w[n], Y])

    L = [A[0].new_ones((A[0].shape[0], 1, A[0].shape[0]))]
    for n in range(N - 1):
        L.append(step(L[n], A[n], n, A[n]))
    R = [None] * N + [A[-1].new_ones((A[-1].shape[2], 1, A[-1].shape[2]))]
    for n in range(N - 1, 0, -1):  # the same step on the mirrored core [r', I, r]
        At = A[n].permute(2, 1, 0).contiguous()
        R[n] = step(R[n + 1], At, n, At)

    def close(W, n):
        return ops.dense_dot(W.contiguous(), R[n + 1]).reshape(())

    out = {}
    for i in range(N):
        out[(i, i)] = close(step(L[i], D[i], i, D[i]), i)
        if not full or i == N - 1:
            continue
        W = step(L[i], D[i], i, A[i])
        for j in range(i + 1, N):
            out[(i, j)] = close(step(W, A[j], j, D[j]), j)
            if j < N - 1:
                W = step(W, A[j], j, A[j])
    return out


def dgsm(t, bounds, marginals=None):
    """Derivative-based global sensitivity measures (derivatives.py:204-235; Kucherenko and Iooss, 2016):
    nu_n = <g_n * pdf, g_n>, g_n = partial(t, n), pdf the product of the marginals, each normalised to sum 1 (``None``: uniform).
    Computed from left / right environments, at most 3 N ``hsum_step`` calls; no gradient train and no product train is built.
    Returns a vector of N entries on ``t``'s device, in its dtype, without a host synchronisation.

    Unlike the reference: the marginals are normalised on a copy (the reference divides the caller's vectors in place); wrong
    lengths raise ValueError; otherwise see the module docstring.
    """
    e = _sensitivity(t, bounds, marginals, False, False, "dgsm")
    return torch.stack([e[(n, n)] for n in range(t.dim())])


def active_subspace(t, bounds, marginals=None):
    """Active subspace (derivatives.py:160-201; Constantine et al., 2017): the eigenpairs, in descending order, of
    M[i, j] = <g_i * pdf, g_j>, with the reference's midpoint weights ((m[:-1] + m[1:]) / 2, normalised, a trailing zero).
    M comes from the environment recursion (at most N^2 + 3 N ``hsum_step`` calls on r x r interfaces instead of N gradient
    trains and N (N + 1) / 2 dots of rank-r^2 product trains) and is assembled on the device in one stack; its N x N
    eigendecomposition is ``torch.linalg.eigh`` on a CPU fp64 copy.  Returns ``(w, v)`` on ``t``'s device, in its dtype.

    Unlike the reference: see ``dgsm`` and the module docstring.
    """
    return _eigenpairs(_as_matrix(t, bounds, marginals), t)


def _as_matrix(t, bounds, marginals):
    """The matrix M of ``active_subspace`` [N, N], on the device."""
    e = _sensitivity(t, bounds, marginals, True, True, "active_subspace")
    N = t.dim()
    return torch.stack([e[(min(i, j), max(i, j))] for i in range(N) for j in range(N)]).reshape(N, N)


def _eigenpairs(M, t):
    c0 = t.cores[0]
    w, v = torch.linalg.eigh(M.to(device="cpu", dtype=torch.float64))
    return w.flip(0).to(device=c0.device, dtype=c0.dtype), v.flip(1).to(device=c0.device, dtype=c0.dtype)

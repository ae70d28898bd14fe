"""Tensor trains from samples (interpolation.py:9-630): ``als_completion`` builds a tensor train from P samples ``y`` at the
integer positions ``X`` by alternating least squares, ``sparse_tt_svd`` (below) by a TT-SVD of the sparse tensor that holds them,
and ``PCEInterpolator`` (last) fits a sparse polynomial to P samples at FLOAT positions and casts it into a TT-Tucker tensor.

``als_completion``

Same signature, defaults, contract and printout as the reference, with three deliberate differences:

1. The core update is the true least-squares minimiser.  The reference orders the columns of its design matrix as (b of R, a of
   L) and reshapes the solution as (a, b), so every core whose two ranks both exceed 1 comes out transposed or scrambled (its
   results are right for N = 2 and for trains with a rank-1 bond next to every interior core only).  Here column a r1 + b holds
   L[a] R[b], so the solution reshapes directly to ``core[:, i, :]``.  (The reference's per-sweep ``eps`` also uses
   ``A.matmul(sol)[0] - b``; here it is the weighted residual of every sample after the sweep's last core update.)
2. A slice whose system is rank-deficient (fewer samples than ``K = r0 r1``, or a degenerate design) gets the minimum-norm
   solution: ``lstsq(..., driver="gelsd")`` on the CPU, ``V diag(lambda+) V^T h`` of its normal equations on the device.  For
   full-rank slices this is the reference's solution up to rounding.
3. Negative indices in ``X`` raise ``ValueError``.

CPU trains run the reference's operator sequence (per-slice lstsq, einsum interface updates) with each mode's samples grouped
once by a stable argsort.  Device trains run, per core step, ``ttr_als_normal`` (the per-slice normal equations on the matrix
cores), ``ttr_spd_solve`` (batched Cholesky; flagged slices go through ``ttr_eigh_trunc`` + ``ttr_gemm`` + ``ttr_pinv_finish``),
the HIP orthogonalisation and one ``ttr_gather_step`` for the interface update; nothing is read back within the sweeps except,
with ``verbose``, one value per sweep.  Batched ``x0`` and autograd are out of scope.

``sparse_tt_svd`` (interpolation.py:122-218) is the TT-SVD of the tensor that holds the samples and zeros elsewhere; its relative
error is at most ``eps``.  Same signature and defaults as the reference, with four deliberate differences:

1. The cores live on ``y``'s device and in ``y``'s dtype (the reference casts through the default dtype).
2. The rank of a bond is also capped by the number of columns (distinct index suffixes) of its unfolding.  The reference keeps up
   to ``nrows`` directions; the extra ones are null vectors of the Gram matrix.
3. Negative indices, and indices ``>= shape[n]`` when ``shape`` is given, raise ``ValueError``.
4. Repeated positions raise ``ValueError`` (the reference lets the last write win, which has no defined order on a GPU).

The samples are sorted once (x_N the major key, x_1 the minor one); in that order the columns of every step are contiguous runs
whose entries ascend in the step's mode index.  CPU trains then run the reference's operator sequence per step (the dense matrix
D of the unfolding, ``D D^T``, ``torch.linalg.eigh``, its rank rule, ``left^T D``).  Device trains never build D: per step
``ttr_sparse_gram`` (work proportional to sum_c m_c^2 r^2 over the columns' entry counts m_c), the HIP eigensolver with the rank
rule on the device, one readback of the selected rank, and ``ttr_sparse_project``.  Batched output and autograd are out of
scope.

``PCEInterpolator`` (interpolation.py:347-630) with its helpers ``get_bounding_box``, ``features2indices``, ``indices2features``,
``empirical_marginals`` and ``gram_schmidt``: sparse polynomial-chaos regression of scattered samples ``(X [P, N], y [P])``.  Same
names, arguments, defaults, algorithm and printout as the reference, and for the same seed the same train / validation rows.
Nothing of ``fit`` that scales with P leaves the device: the moment matrices ``H_n = V_n^T V_n / P`` of all modes are one
reduction in fp64 (one readback of ``[N, S, S]``), the reference's modified Gram-Schmidt runs on them on the host with the inner
product ``u^T H v`` (the reference makes S^2 passes over the samples per mode), the design matrix is one ``ttr_pce_design``
launch, LARS (``_lars.py``) walks its path on the host in fp64 from the Gram matrix ``M^T M`` and ``M^T y`` alone (``ttr_gemm``, one copy to the host;
the basis is orthonormal under the empirical measure, so the Gram matrix is well conditioned), and the validation error of the
whole path is one GEMM.  ``predict`` is one ``ttr_pce_predict`` launch and never forms the P x C matrix.  CPU tensors run the
same class through the mirrors in ``_hostops``.  Deliberate differences:

1. No scikit-learn anywhere.  The LARS here follows scikit-learn's path (checked against it to 1e-12 of the path's largest
   entry), but goes on until ``max|c| / P_train <= 2.2e-16`` where scikit-learn stops at the fp32 epsilon.
2. Results are in ``X``'s dtype (fp32 or fp64) on ``X``'s device (the reference casts through ``torch.Tensor``: fp32 on the CPU).
3. Invalid arguments raise ``ValueError`` where the reference fails an ``assert``: ``X`` not 2-D or not fp32 / fp64, ``y`` of
   the wrong length, ``q`` outside ``(0, 1]`` (``q = 0`` included), a ``domain`` or ``bbox`` of the wrong length, and
   ``int(P * val_split) < 1`` (the reference divides by the norm of an empty vector there).  On a device, ``ceil(p)`` above
   ``ttr_pce_max_order()`` (16) or ``N * ceil(p)`` above ``ttr_pce_max_basis()`` (256) raise ``ValueError`` too.
4. ``features2indices(domain=...)`` interpolates with torch on the input's device, for any leading shape (the reference goes
   through ``np.interp`` on 2-D CPU input).
5. ``empirical_marginals`` uses ``features2indices(domain=)`` (the reference calls a ``tn.discretize`` that does not exist) and
   returns vectors in ``X``'s dtype.
6. ``retrain=False`` also sets ``allcoords`` (and ``allcoef``).
7. ``Psis`` is one ``[N, S, S]`` tensor (indexing it gives the reference's list entries).
"""

from __future__ import annotations

import math
import time

import numpy as np
import torch

__all__ = ["als_completion", "sparse_tt_svd", "get_bounding_box", "features2indices", "indices2features", "empirical_marginals",
           "gram_schmidt", "PCEInterpolator"]

_STEP_HOOK = None  # diagnostics: called with n after step n of sparse_tt_svd (memory / time per step)
MAX_DEVICE_K = 1024  # r0 * r1 of a core: ttr_als_normal / ttr_spd_solve's limit


def als_completion(X, y, ranks_tt, shape=None, ws=None, x0=None, niter=10, verbose=True):
    """Complete an N-dimensional TT from P samples by alternating least squares (interpolation.py:9-119).

    Every tensor slice needs at least one sample (the usual case for categorical variables).  Convergence may be slow or fail
    when the samples are few compared to the tensor (M. Steinlechner, "Riemannian optimization for high-dimensional tensor
    completion", 2015).  Unlike the reference, each core update is the exact least-squares minimiser, rank-deficient slices get
    the minimum-norm solution, and negative indices raise ``ValueError`` (see the module docstring).

    :param X: a P x N matrix of integers (tensor indices)
    :param y: a vector with P elements
    :param ranks_tt: an integer (or list).  Ignored if ``x0`` is given
    :param shape: list of N integers.  If None, the smallest shape that accommodates ``X`` will be chosen
    :param ws: a vector with P elements, the weight of each sample (None: 1); the objective is sum (w_p (a_p x - y_p))^2
    :param x0: initial solution (a TT tensor; its cores list is rebound, their storage is never written).  If None, a random
        tensor (``tn.rand``, drawn on the CPU in the default dtype) moved to ``y``'s device
    :param niter: number of ALS sweeps.  Default is 10
    :param verbose: print one line per sweep with eps = ||w (y - t[X])|| / ||y||
    :return: ``x0`` (a :class:`Tensor`)
    """
    from .create import rand
    from .tensor import Tensor

    assert not X.dtype.is_floating_point
    assert X.dim() == 2
    assert y.dim() == 1
    P, N = X.shape
    if N < 2:
        raise ValueError("als_completion needs at least two modes")
    X = X.long()
    if P > 0 and int(X.min()) < 0:
        raise ValueError("als_completion: negative indices in X")
    if shape is None:
        shape = [int(v) for v in (torch.max(X, dim=0)[0] + 1).tolist()]
    if x0 is None:
        x0 = rand(shape, ranks_tt=ranks_tt)
        if y.device.type != "cpu":
            x0.cores = [c.to(y.device) for c in x0.cores]
    if x0.batch:
        raise NotImplementedError("als_completion: batched x0 is not supported")
    device, dtype = x0.cores[0].device, x0.cores[0].dtype
    on_dev = device.type != "cpu"
    Is = [int(s) for s in x0.shape]
    X = X.to(device)
    y = y.to(device=device, dtype=dtype)
    w = torch.ones(P, dtype=dtype, device=device) if ws is None else torch.as_tensor(ws).to(device=device, dtype=dtype)

    # All tensor slices must contain at least one sample point; each mode's samples grouped once (stable)
    counts = [torch.bincount(X[:, n], minlength=Is[n]) for n in range(N)]
    sizes = [int(c.numel()) for c in counts]
    counts = torch.cat(counts).tolist()
    cnt, pos = [], 0
    for n in range(N):
        if sizes[n] != Is[n]:
            raise ValueError("als_completion: index {} out of range for mode {} of size {}".format(sizes[n] - 1, n, Is[n]))
        cnt.append(counts[pos : pos + Is[n]])
        pos += Is[n]
    if any(c == 0 for cn in cnt for c in cn):
        raise ValueError("One groundtruth sample is needed for every tensor slice")
    xs = [X[:, n].contiguous() for n in range(N)]
    orders = [torch.sort(xs[n], stable=True).indices for n in range(N)]

    if verbose:
        print("Completing a {}D tensor of size {} using {} samples...".format(N, list(shape), P))

    x0.orthogonalize(0)
    if on_dev:
        from . import _hip, _hipops
        from ._dispatch import ops_for

        ops_for(x0.cores[0])  # the library and the dtype, checked up front
        Ks = [int(c.shape[0]) * int(c.shape[2]) for c in x0.cores]
        if max(Ks) > MAX_DEVICE_K:
            raise NotImplementedError(
                "als_completion: r0 * r1 = {} exceeds the device limit of {} (ranks up to 32)".format(max(Ks), MAX_DEVICE_K))
        plans = {}

        def plan(n, K):
            if (n, K) not in plans:
                plans[(n, K)] = _hipops.AlsPlan(cnt[n], K, y.element_size(), device)
            return plans[(n, K)]

        def core_update(mu):
            L, R = lefts[mu], rights[mu]
            return _hipops.als_core(L, R, w if ws is not None else None, y, orders[mu], plan(mu, L.shape[1] * R.shape[1]), Is[mu])

        def left_step(L, core, x):
            return _hip.gather_step(L, None, core, x)

        def right_step(R, core, x):
            return _hip.gather_step(R, None, core.permute(2, 1, 0), x)

    else:
        from . import _hostops

        offs = []
        for n in range(N):
            off = [0]
            for c in cnt[n]:
                off.append(off[-1] + c)
            offs.append(off)

        def core_update(mu):
            return _hostops.als_core(lefts[mu], rights[mu], w, y, orders[mu], offs[mu], Is[mu])

        left_step, right_step = _hostops.als_left_step, _hostops.als_right_step

    # Memoized product chains of all samples, [P, r]: lefts are filled on the go, rights now (interpolation.py:60-70)
    lefts = [torch.ones(P, int(x0.cores[0].shape[0]), dtype=dtype, device=device)] + [None] * (N - 1)
    rights = [None] * (N - 1) + [torch.ones(P, int(x0.cores[-1].shape[2]), dtype=dtype, device=device)]
    for n in range(N - 2, -1, -1):
        rights[n] = right_step(rights[n + 1], x0.cores[n + 1], xs[n + 1])
    normy = torch.sqrt((y * y).sum()) if verbose else None

    def set_core(mu, core):
        x0.cores = x0.cores[:mu] + [core] + x0.cores[mu + 1 :]

    start = time.time()
    for swp in range(niter):
        for mu in range(N - 1):  # left to right
            set_core(mu, core_update(mu))
            x0.left_orthogonalize(mu)
            lefts[mu + 1] = left_step(lefts[mu], x0.cores[mu], xs[mu])
        for mu in range(N - 1, 0, -1):  # right to left
            set_core(mu, core_update(mu))
            x0.right_orthogonalize(mu)
            rights[mu - 1] = right_step(rights[mu], x0.cores[mu], xs[mu])
        if verbose:
            vals = (left_step(lefts[0], x0.cores[0], xs[0]) * rights[0]).sum(dim=1)
            res = w * (y - vals)
            eps = float(torch.sqrt((res * res).sum()) / normy)
            print("iter: {: <{}}".format(swp, len("{}".format(niter)) + 1), end="")
            print("| eps: {:.3e}".format(eps), end="")
            print(" | time: {:8.4f}".format(time.time() - start))

    return x0


def sparse_tt_svd(X, y, eps, shape=None, rmax=None):
    """TT-SVD for sparse tensors (interpolation.py:122-218): the tensor train of the tensor that holds ``y`` at the positions
    ``X`` and zeros elsewhere.

    Unlike the reference, the cores live on ``y``'s device and in ``y``'s dtype, the rank of a bond is also capped by the number
    of columns of its unfolding, and bad indices (negative, or ``>= shape[n]`` for a given ``shape``) and repeated positions
    raise ``ValueError`` (see the module docstring).  A mode index without a sample is a zero slice.  On a device every step's
    unfolding needs ``rank * shape[n] <= 4096`` (fp32) / 2048 (fp64) rows; beyond that ``NotImplementedError`` names the bond.
    With a finite ``rmax`` that check runs before any work on the WORST case ``min(rmax, rows, P) * shape[n]``, so a generous
    ``rmax`` can refuse an input that ``rmax=None`` (checked step by step, on the ranks ``eps`` really selects) decomposes.  The
    device eigensolver's zero guard treats ``sigma_max < 1e-13`` (absolute) as zero: samples that small give rank 1 whatever
    ``eps`` is; scale ``y`` first.

    :param X: matrix P X N of sample coordinates (integers; a torch tensor or a NumPy array)
    :param y: P-sized vector of sample values (a torch tensor or a NumPy array)
    :param eps: prescribed accuracy (resulting relative error is guaranteed to be not larger than this)
    :param shape: input tensor shape. If not specified, a tensor will be chosen such that `X` fits in
    :param rmax: optionally, cap all ranks above this value
    :return: a TT (a :class:`Tensor`)
    """
    from .tensor import Tensor

    X, y = torch.as_tensor(X), torch.as_tensor(y)
    assert not X.dtype.is_floating_point
    assert X.dim() == 2
    assert y.dim() == 1 and y.dtype.is_floating_point
    P, N = X.shape
    if N < 2:
        raise ValueError("sparse_tt_svd needs at least two modes")
    if P == 0:
        raise ValueError("sparse_tt_svd needs at least one sample")
    assert y.shape[0] == P
    device, dtype = y.device, y.dtype
    on_dev = device.type != "cpu"
    X = X.to(device).long()
    if shape is None:
        shape = (torch.max(X, dim=0)[0] + 1).tolist()
        if min(shape) < 1:
            raise ValueError("sparse_tt_svd: negative indices in X")
    shape = [int(s) for s in shape]
    assert N == len(shape)
    if min(shape) < 1:
        raise ValueError("sparse_tt_svd: empty mode in shape {}".format(shape))
    if rmax is None:
        rmax = 2**31 - 1
    rmax = max(1, int(rmax))

    if on_dev:
        from . import _hip
        from . import _hipops as ops

        limit = _hip.max_eigh_n(dtype)
        if rmax < 2**31 - 1:  # the bound is known in advance: before any work
            bound = 1
            for n in range(N - 1):
                if bound * shape[n] > limit:
                    raise NotImplementedError(_ENVELOPE.format(n + 1, bound, shape[n], bound * shape[n], limit, dtype))
                bound = min(rmax, bound * shape[n], P)
        # delta^2 = (eps / sqrt(N - 1) ||y||)^2 stays on the device (the rank rule reads it there)
        delta = (_hip.norm(y.contiguous()[None]).double() ** 2) * (float(eps) ** 2 / (N - 1))
    else:
        from . import _hostops as ops

        delta = float(eps) / (N - 1) ** 0.5 * float(torch.norm(y))

    perm, lev = ops.sparse_canonical(X, shape)
    V = y[perm][:, None].contiguous()  # [blocks, r]: the blocks of step 1 are the sorted samples, r = 1
    first = None  # sorted position of the first sample of every block (None: every sample is a block)
    cores = []
    for n in range(1, N):
        I, r, nb = shape[n - 1], V.shape[1], V.shape[0]
        if on_dev and r * I > limit:
            raise NotImplementedError(_ENVELOPE.format(n, r, I, r * I, limit, dtype))
        mark = lev >= n + 1  # a new column of this step (a new suffix x_{n+1..N}) starts at these sorted samples
        start = torch.nonzero(mark)[:, 0].to(torch.int32)
        C = int(start.shape[0])
        i32 = torch.int32  # the block table travels as int32 (P < 2^31)
        xn = X[:, n - 1].to(i32)
        if first is None:
            blk_i, blkcol, ptr = xn[perm], torch.cumsum(mark, dim=0, dtype=i32) - 1, start
        else:
            blk_i, blkcol = xn[perm[first]], torch.cumsum(mark[first], dim=0, dtype=i32) - 1
            ptr = torch.searchsorted(first, start, out_int32=True)
        del xn
        colptr = torch.cat([ptr, torch.full((1,), nb, dtype=i32, device=device)])
        del mark
        left, V = ops.sparse_step(V, I, colptr, blk_i.contiguous(), blkcol, delta, min(rmax, r * I, C))
        cores.append(left.reshape(r, I, left.shape[1]).contiguous())
        first = start
        if _STEP_HOOK is not None:
            _STEP_HOOK(n)
    last = torch.zeros(V.shape[1], shape[-1], 1, dtype=dtype, device=device)
    last[:, X[:, N - 1][perm[first]], 0] = V.t()
    cores.append(last)
    return Tensor(cores)


_ENVELOPE = ("sparse_tt_svd: the unfolding of bond {} has rank {} x size {} = {} rows, above the device limit of {} for {}")


def get_bounding_box(X):
    """Smallest and largest value of every feature (interpolation.py:221-232).

    :param X: tensor ``[..., N]``; the last axis runs over the N features
    :return: N pairs ``(min, max)`` of Python floats
    """
    flat = X.reshape(-1, X.shape[-1])
    lo, hi = flat.min(dim=0)[0].tolist(), flat.max(dim=0)[0].tolist()
    return list(zip(lo, hi))


def _check_len(what, seq, N):
    if len(seq) != N:
        raise ValueError("{} must have one entry per feature ({}), got {}".format(what, N, len(seq)))


def features2indices(X, bbox=None, I=512, domain=None):
    """Nearest grid index of every feature value (interpolation.py:235-264).

    With ``domain`` (N ascending grid vectors; it takes precedence over ``bbox`` and ``I``) a value's position in its grid is
    interpolated linearly between the two grid points around it, held at the ends, and rounded.  Without it the grid is ``I``
    equispaced points from ``bbox[n][0]`` to ``bbox[n][1]`` (``bbox`` None: X's own bounding box) and values beyond the box land
    on its first or last index.  Runs with torch on X's device, for any leading shape.

    :param X: floating-point tensor ``[..., N]``
    :param bbox: N pairs ``(bottom, top)``, or None
    :param I: number of grid points per feature (512 by default)
    :param domain: N grid vectors, or None
    :return: int64 tensor of X's shape
    """
    if not (torch.is_tensor(X) and X.dtype.is_floating_point and X.dim() >= 1):
        raise ValueError("features2indices: X must be a floating-point tensor of shape ... x N")
    N = X.shape[-1]
    if domain is not None:
        _check_len("features2indices: domain", domain, N)
        out = torch.empty_like(X)
        for n in range(N):
            xs = torch.as_tensor(domain[n]).to(device=X.device, dtype=X.dtype).contiguous()
            x = X[..., n].contiguous()
            if xs.shape[0] < 2:
                out[..., n] = 0
                continue
            j = (torch.searchsorted(xs, x, right=True) - 1).clamp(0, xs.shape[0] - 2)   # the grid cell of every value
            val = (1.0 / (xs[j + 1] - xs[j])) * (x - xs[j]) + j.to(X.dtype)
            out[..., n] = val.clamp(0, xs.shape[0] - 1)
        return torch.round(out).long()
    if bbox is None:
        bbox = get_bounding_box(X)
    _check_len("features2indices: bbox", bbox, N)
    bbox = torch.as_tensor(bbox, dtype=X.dtype, device=X.device)
    X = (X - bbox[:, 0]) / (bbox[:, 1] - bbox[:, 0])
    return torch.round(X * (I - 1)).long().clamp(0, I - 1)


def indices2features(X, bbox=None, I=512, domain=None):
    """Grid value at every index: the way back from ``features2indices`` (interpolation.py:267-281).

    The grid of feature n is ``domain[n]`` when ``domain`` is given; otherwise the centres of ``I`` equal cells of
    ``bbox[n]``, built in the default dtype.

    :param X: integer matrix ``[P, N]``
    :param bbox: N pairs ``(bottom, top)``; required without ``domain``
    :param I: cells per feature (512 by default)
    :param domain: N grid vectors, or None
    :return: ``[P, N]`` on X's device, in the grid's dtype
    """
    if not (torch.is_tensor(X) and not X.dtype.is_floating_point and X.dim() == 2):
        raise ValueError("indices2features: X must be an integer P x N matrix")
    N = X.shape[1]
    if domain is None:
        if bbox is None:
            raise ValueError("indices2features: one of bbox and domain is needed")
        _check_len("indices2features: bbox", bbox, N)
        domain = [_cell_centres(b, I) for b in bbox]
    _check_len("indices2features: domain", domain, N)
    domain = [torch.as_tensor(d).to(X.device) for d in domain]
    result = torch.zeros(X.shape, dtype=domain[0].dtype if N else torch.get_default_dtype(), device=X.device)
    for n in range(N):
        result[:, n] = domain[n][X[:, n].long()]
    return result


def _cell_centres(b, I, **kw):
    """Centres of I equal cells of the interval b = (bottom, top) (interpolation.py:273-277, 584-592)."""
    half = (b[1] - b[0]) / (2 * I)
    return torch.linspace(b[0] + half, b[1] - half, I, **kw)


def empirical_marginals(X, domain):
    """Share of the P samples that falls on every grid point, feature by feature (interpolation.py:284-304; the reference
    calls a ``tn.discretize`` that does not exist, this goes through ``features2indices(domain=)``).

    :param X: floating-point matrix ``[P, N]``
    :param domain: N grid vectors
    :return: N vectors (``len(domain[n])`` entries summing to 1) in X's dtype on X's device
    """
    if not (torch.is_tensor(X) and X.dim() == 2 and X.dtype.is_floating_point):
        raise ValueError("empirical_marginals: X must be a floating-point P x N matrix")
    P, N = X.shape
    _check_len("empirical_marginals: domain", domain, N)
    Xd = features2indices(X, domain=domain)
    return [torch.bincount(Xd[:, n], minlength=len(domain[n])).to(X.dtype) / P for n in range(N)]


def _gram_schmidt_moments(H):
    """Modified Gram-Schmidt on the monomials 1, x, .., x^(S-1) under the measure whose moment matrix is H [S, S] (NumPy, fp64):
    ``<u, v> = u^T H v`` for coefficient vectors.  Column s starts as e_s, loses its components along columns 0 .. s - 1 one
    after the other (each computed on the already reduced vector), then is normalised -- the order of operations of
    interpolation.py:337-344; column 0 stays e_0."""
    S = H.shape[0]
    Psi = np.eye(S)
    for s in range(1, S):
        u = Psi[:, s].copy()
        for k in range(s):
            a = Psi[:, k]
            u = u - (a @ H @ u) / (a @ H @ a) * a
        Psi[:, s] = u / np.sqrt(u @ H @ u)
    return Psi


def gram_schmidt(x, S):
    """S polynomials of degree 0 .. S - 1 that are orthonormal under the empirical measure of the samples ``x``
    (interpolation.py:307-344; Witteveen and Bijl, "Modeling Arbitrary Uncertainties Using Gram-Schmidt Polynomial Chaos", 2012).

    The samples are read once, for the moment matrix ``H[j, k] = mean(x^(j + k))`` in fp64; modified Gram-Schmidt then runs on
    H on the host (the reference passes over the samples for every inner product).

    :param x: floating-point vector of samples
    :param S: number of polynomials
    :return: ``[S, S]`` in x's dtype on x's device, upper triangular: column s holds the monomial coefficients of polynomial s
    """
    if not (torch.is_tensor(x) and x.dim() == 1 and x.dtype.is_floating_point):
        raise ValueError("gram_schmidt: x must be a floating-point vector")
    from ._dispatch import ops_for

    H = ops_for(x).pce_moments(x[:, None], int(S))[0].cpu().numpy()
    return torch.as_tensor(_gram_schmidt_moments(H)).to(device=x.device, dtype=x.dtype)


def _hyperbolic_candidates(N, S, p, q, max_count, limit):
    """All multi-indices of [0, S)^N with ``sum_n idx_n^q < p^q``, in lexicographic order, as an int64 array [C, N]: the
    candidate set of interpolation.py:452-478.  A depth-first walk over the modes: a term never lowers the sum, so a prefix
    that fails with zeros behind it ends its level.  The test itself is the NumPy expression on the whole int64 index vector,
    so a borderline index falls on the reference's side.  More than ``max_count`` candidates raise the reference's error."""
    bound = p**q
    idx = np.zeros(N, dtype=np.int64)
    found = []

    def walk(n):
        for s in range(S):
            idx[n] = s
            if not np.sum(idx**q) < bound:
                break
            if n + 1 < N:
                walk(n + 1)
                continue
            found.append(idx.copy())
            if len(found) > max_count:
                raise ValueError(
                    "Design matrix exceeds matrix_size_limit ({:g} elements). Decrease p or q, or increase matrix_size_limit".format(limit))
        idx[n] = 0

    walk(0)
    return np.array(found, dtype=np.int64).reshape(len(found), N)


class PCEInterpolator:
    """Sparse polynomial-chaos regression of scattered samples (interpolation.py:347-630): a surrogate
    ``y(x) ~ sum_c coef[c] prod_n psi_{n, coords[c, n]}(x_n)`` of ``(X [P, N], y [P])``.

    The polynomials of feature n are orthonormal under the empirical distribution of that feature (``gram_schmidt``; no
    distribution is assumed, the features are treated as independent).  The candidates are the multi-indices with
    ``||idx||_q < p`` (hyperbolic truncation); least angle regression orders them, and a validation split picks how many stay
    (Torre et al., "Data-driven Polynomial Chaos Expansion for Machine Learning Regression", 2020).

    Everything follows the device and dtype (fp32 or fp64) of the ``X`` given to ``fit``; the module docstring says what runs
    where and how this differs from the reference.  ``fit`` leaves behind ``bbox``, ``X_mean``, ``X_std``, ``Psis`` ([N, S, S]),
    ``allcoords`` / ``allcoef`` (every candidate) and ``coords`` / ``coef`` (the selected ones).
    """

    def __init__(self):
        pass

    def _centred(self, X):
        if not (torch.is_tensor(X) and X.dim() == 2 and X.shape[1] == self.X_mean.shape[0]):
            raise ValueError("PCEInterpolator: X must be a P x {} matrix".format(self.X_mean.shape[0]))
        X = X.to(device=self.X_mean.device, dtype=self.X_mean.dtype)
        return (X - self.X_mean[None, :]) / self.X_std[None, :]

    def fit(self, X, y, p=5, q=0.75, val_split=0.1, seed=0, matrix_size_limit=5e7, retrain=True, verbose=True):
        """Select and fit the coefficients on the samples ``(X, y)``.

        :param X: floating-point (fp32 or fp64) matrix ``[P, N]`` of features
        :param y: P target values
        :param p: radius of the hyperbolic truncation; ``ceil(p)`` polynomials per feature
        :param q: exponent of its quasi-norm, in (0, 1]
        :param val_split: share of the samples drawn (with replacement) for validation
        :param seed: seed of that draw
        :param matrix_size_limit: refuse design matrices of more than this many entries
        :param retrain: once the number of terms is chosen, run LARS again on all samples (True), or keep the coefficients
            the training rows gave (False: cheaper, for parameter scans)
        :param verbose: print the reference's progress lines
        """
        from . import _lars
        from ._dispatch import ops_for

        if not (torch.is_tensor(X) and X.dim() == 2 and X.dtype in (torch.float32, torch.float64)):
            raise ValueError("PCEInterpolator.fit: X must be an fp32 or fp64 P x N matrix")
        P, N = X.shape
        if not (torch.is_tensor(y) and y.dim() == 1 and y.shape[0] == P):
            raise ValueError("PCEInterpolator.fit: y must be a vector of {} elements".format(P))
        if not 0 < q <= 1:
            raise ValueError("PCEInterpolator.fit: q must lie in (0, 1], got {}".format(q))
        n_val = int(P * val_split)
        if n_val < 1:
            raise ValueError("PCEInterpolator.fit: int(P * val_split) = {} leaves no validation sample".format(n_val))
        ops = ops_for(X)
        device, dtype = X.device, X.dtype
        S = int(math.ceil(p))
        if device.type != "cpu":
            max_order, max_basis = ops.pce_limits()
            if S > max_order or N * S > max_basis:
                raise ValueError("PCEInterpolator.fit: ceil(p) = {} and N * ceil(p) = {} exceed the device limits {} and {}".format(
                    S, N * S, max_order, max_basis))
        y = y.to(device=device, dtype=dtype)

        # standardised features: the powers in the moment matrices stay of order one
        self.bbox = get_bounding_box(X)
        self.X_mean = torch.mean(X, dim=0)
        self.X_std = torch.std(X, dim=0)
        Z = (X - self.X_mean[None, :]) / self.X_std[None, :]

        # the reference's rows for this seed: n_val draws with replacement validate, every row never drawn trains
        drawn = np.random.default_rng(seed=seed).choice(P, n_val)
        idx_train = torch.as_tensor(np.delete(np.arange(P), drawn), device=device)
        idx_val = torch.as_tensor(drawn, device=device)

        start = time.time()
        if verbose:
            print("PCE interpolation (p={}, q={}) of {} points ({} train + {} val) in {}D".format(p, q, P, P - n_val, n_val, N))
            print("{:.3f}s | ".format(time.time() - start), end="")
            print("Hyperbolic truncation...", end="")

        allcoords = torch.as_tensor(_hyperbolic_candidates(N, S, p, q, matrix_size_limit / P, matrix_size_limit), device=device)
        C = int(allcoords.shape[0])

        if verbose:
            print(" done, we kept {} / {} candidates".format(C, S**N))
            print("{:.3f}s | ".format(time.time() - start), end="")
            print("Assembling a {} X {} design matrix...".format(P, C), end="", flush=True)

        # bases from the moment matrices of all modes (one reduction, one readback), then the design matrix in one launch
        H = ops.pce_moments(Z, S).cpu().numpy()
        self.Psis = torch.as_tensor(np.stack([_gram_schmidt_moments(H[n]) for n in range(N)])).to(device=device, dtype=dtype)
        M = ops.pce_design(Z, self.Psis, allcoords)
        M_val, y_val = M[idx_val], y[idx_val]

        if verbose:
            print(" done")
            print("{:.3f}s | ".format(time.time() - start), end="")
            print("Finding best nnz in LARS...", end="", flush=True)

        # LARS sees the train rows through their normal equations only
        Gb = ops.pce_gram(M[idx_train], y[idx_train]).cpu()    # [C + 1, C]: M^T M over M^T y, one copy
        path, _ = _lars.lars_path(Gb[:C], Gb[C], n_samples=int(idx_train.shape[0]))

        # validation error of every column of the path at once; the first minimum fixes the number of terms
        reco_path = ops.mm(M_val[None], torch.as_tensor(path).to(device=device, dtype=dtype).contiguous()[None])[0]
        error_path = (torch.sqrt(torch.sum((reco_path - y_val[:, None]) ** 2, dim=0)) / torch.norm(y_val)).cpu()
        argmin = int(torch.argmin(error_path))
        nnz = int(np.count_nonzero(path[:, argmin]))

        if verbose:
            print(" done, val eps={:.5g}".format(float(error_path[argmin])))
            print("{:.3f}s | ".format(time.time() - start), end="")

        if retrain:
            if verbose:
                print("Retraining at nnz={}...".format(nnz), end="", flush=True)
            Gb = ops.pce_gram(M, y).cpu()
            allcoef = _lars.lars_path(Gb[:C], Gb[C], n_samples=P, max_steps=nnz)[0][:, -1]
        else:
            allcoef = path[:, argmin]

        kept = torch.as_tensor(np.flatnonzero(allcoef), device=device)
        self.allcoords = allcoords
        self.allcoef = torch.as_tensor(allcoef).to(device=device, dtype=dtype)
        self.coef = self.allcoef[kept].contiguous()
        self.coords = allcoords[kept, :].contiguous()

        if verbose:
            if retrain:
                reco = ops.mm(M[None], self.allcoef[None, :, None])[0, :, 0]
                print(" done, training eps={:.5g}".format(float(torch.norm(y - reco) / torch.norm(y))))
                print("{:.3f}s".format(time.time() - start), flush=True)
            print()

    def predict(self, X):
        """Values of the fitted surrogate at new points.

        :param X: matrix ``[P, N]`` of features
        :return: P values, on the device and in the dtype of the fit
        """
        from ._dispatch import ops_for

        Z = self._centred(X)
        # (the coordinates are fit's own enumeration: inside [0, S) by construction, so the kernel's flag is not read back)
        return ops_for(Z).pce_predict(Z, self.Psis, self.coords, self.coef, check=False)

    def to_tensor(self, domain=512, rmax=200, eps=1e-3, verbose=True):
        """The surrogate sampled on a grid, as a TT-Tucker tensor: the coefficient tensor in TT form (``sparse_tt_svd``) with
        the polynomials evaluated on the grid as Tucker factors.

        :param domain: N grid vectors, or an integer I: the centres of I equal cells of every feature's range in the fit
        :param rmax: largest TT rank of the coefficient tensor
        :param eps: relative accuracy of its TT-SVD
        :param verbose: print the reference's progress lines
        :return: a :class:`Tensor` of shape ``[len(grid_1), .., len(grid_N)]`` with ``Us`` set
        """
        N, S = int(self.Psis.shape[0]), int(self.Psis.shape[1])
        device, dtype = self.Psis.device, self.Psis.dtype
        if not isinstance(domain, (list, tuple)):
            domain = [_cell_centres(self.bbox[n], domain, dtype=dtype, device=device) for n in range(N)]
        _check_len("PCEInterpolator.to_tensor: domain", domain, N)

        start = time.time()
        if verbose:
            print("Conversion to TT-Tucker format (rmax={}, eps={:.5g})".format(rmax, eps))
            print("{:.3f}s | ".format(time.time() - start), end="")
            print("Sparse TT-SVD...", end="", flush=True)

        t = sparse_tt_svd(self.coords, self.coef, rmax=rmax, eps=eps)

        if verbose:
            err = torch.norm(t[self.coords].torch() - self.coef) / torch.norm(self.coef)
            print(" done, rmax={}, eps={:.5g}".format(max(t.ranks_tt), float(err)))

        # factor n: the polynomials the core's mode n reaches, on the standardised grid
        ks = torch.arange(S, device=device)
        Us = []
        for n in range(N):
            z = (torch.as_tensor(domain[n]).to(device=device, dtype=dtype) - self.X_mean[n]) / self.X_std[n]
            Us.append((z[:, None] ** ks).matmul(self.Psis[n][:, : t.shape[n]]))
        t.Us = Us

        if verbose:
            print("{:.3f}s".format(time.time() - start), flush=True)
            print()

        return t

"""Tensor trains from samples (interpolation.py:9-218): ``als_completion`` builds a tensor train from P samples ``y`` at the
integer positions ``X`` by alternating least squares, ``sparse_tt_svd`` (below) by a TT-SVD of the sparse tensor that holds them.

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
with ``verbose``, one value per sweep.  Batched ``x0``, ``PCEInterpolator`` and autograd are out of scope.

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
rule on the device, one readback of the selected rank, and ``ttr_sparse_project``.  ``PCEInterpolator``, batched output and
autograd are out of scope.
"""

from __future__ import annotations

import time

import torch

__all__ = ["als_completion", "sparse_tt_svd"]

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

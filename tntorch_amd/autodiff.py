"""Gradient-based fitting: ``tn.optimize``, ``tn.dof`` (autodiff.py:10-121) and the differentiable operations of the device path.

The reference leaves differentiation to torch autograd over its einsum chains.  The HIP kernels are opaque to autograd, so the
operations that the fitting losses of the reference's tutorials are made of carry hand-written backward passes here, each one
``torch.autograd.Function`` (grad mode is off inside its ``forward``, so the kernels' work is not recorded; the operands are
passed as they are, not detached copies):

- ``t[X]`` with index arrays on the first k modes (``point_eval``): forward one ``ttr_gather_step`` per mode,
  the left interfaces kept; backward one ``ttr_gather_grad`` per core that needs a gradient (the per-slice sum of outer
  products L[p]^T R[p] on the matrix cores) and one ``ttr_gather_step`` per mode that moves the right interface;
- ``tt_multiply`` (``tt_matvec``): forward the chain of ``ttr_ttm_step``, the step inputs kept for the cores
  that need a gradient; backward one ``ttr_ttm_grad_core`` per such core and one ``ttr_ttm_grad_input`` per step that still has
  an operand before it which needs one, each step's ``dX`` being the previous step's ``dY`` as it lies;
- ``mode_mul`` (Tucker factors), ``gemm`` (the chain of ``Tensor.torch()``) and ``dense_dist`` (``tn.dist`` /
  ``tn.relative_error`` against a dense tensor): existing kernels in both directions.

Everything else keeps refusing device operands that require grad (``Tensor._norm4`` / ``_dispatch.ops_for``), as do batched
trains, CP cores and keys of any other form.  CPU trains need none of this: the host mirror is plain torch.  No double backward.
"""

from __future__ import annotations

import time
from collections import OrderedDict
from typing import List, Optional, Sequence

import torch
from torch.autograd.function import once_differentiable

__all__ = ["optimize", "dof"]

_OOB = "index out of range: an index array entry lies outside its mode"


# ---------------------------------------------------------------------------------------------- grouping plans of index columns
PLAN_BUILDS = 0         # plans built so far (tests: an optimize loop sorts and reads counts back once, not once per iteration)
PLAN_CACHE_SIZE = 16    # least recently used entries beyond this are dropped
TASK_SAMPLES: Optional[int] = None  # samples per ttr_gather_grad task (None: _hostops.GRAD_TASK_SAMPLES); tests split small slices
_plans: "OrderedDict[int, tuple]" = OrderedDict()
_plan_serial = 0


def _plan_key(col: torch.Tensor, I: int):
    return (col.storage_offset(), tuple(col.stride()), tuple(col.shape), col.dtype, col._version, int(I), TASK_SAMPLES)


def build_plan(col: torch.Tensor, I: int):
    """(perm, GradPlan) of one validated index column: indices wrapped, sample numbers sorted by slice (stable), per-slice counts
    read back once."""
    global PLAN_BUILDS
    from . import _hostops

    PLAN_BUILDS += 1
    v = torch.remainder(col, I)
    perm = torch.sort(v, stable=True).indices
    counts = torch.bincount(v, minlength=I).cpu().tolist() if col.shape[0] else [0] * I
    return perm, _hostops.GradPlan(counts, col.device, TASK_SAMPLES)


def plan_for(col: torch.Tensor, I: int, cache: bool = True):
    """The plan of ``col``, reused while the same unmodified tensor is passed again: an entry holds the base tensor object itself
    (so its identity cannot be recycled) and matches on that object, the view's offset, strides and length, and the version
    counter that every in-place write bumps.  Never on a bare data pointer."""
    global _plan_serial
    if not cache:
        return build_plan(col, I)
    base = col._base if col._base is not None else col
    key = _plan_key(col, I)
    for serial, (b, k, value) in _plans.items():
        if b is base and k == key:
            _plans.move_to_end(serial)
            return value
    value = build_plan(col, I)
    _plan_serial += 1
    _plans[_plan_serial] = (base, key, value)
    while len(_plans) > PLAN_CACHE_SIZE:
        _plans.popitem(last=False)
    return value


def clear_plans() -> None:
    _plans.clear()


# ---------------------------------------------------------------------------------------------- t[X]
class _PointEval(torch.autograd.Function):
    """out [1, P, r_k] = prod_n cores[n][:, cols[n][p], :] for cores [r_n, I_n, r_{n+1}] with r_0 = 1."""

    @staticmethod
    def forward(ctx, cols, cacheable, *cores):
        from . import _hip

        dev, dt = cores[0].device, cores[0].dtype
        k, P = len(cores), cols[0].shape[0]
        flags = torch.zeros(k, dtype=torch.int32, device=dev)
        Ls = [torch.ones((P, 1), dtype=dt, device=dev)]
        for n in range(k):
            if P == 0:  # nothing to evaluate (and an empty tensor has no address to pass)
                Ls.append(torch.empty((0, cores[n].shape[2]), dtype=dt, device=dev))
            else:
                Ls.append(_hip.gather_step(Ls[-1], None, cores[n], cols[n], flag=flags[n:n + 1]))
        if P and int(flags.max().item()):  # the one host read of the call
            raise IndexError(_OOB)
        needs = [bool(x) for x in ctx.needs_input_grad[2:]]
        ctx.plans = [plan_for(cols[n], cores[n].shape[1], cacheable[n]) if needs[n] else None for n in range(k)]
        ctx.cols = cols
        ctx.save_for_backward(*cores, *Ls[:k])
        return Ls[k].reshape(1, P, cores[-1].shape[2])

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        from . import _hip, _hipops

        k = len(ctx.cols)
        cores, Ls = ctx.saved_tensors[:k], ctx.saved_tensors[k:]
        needs = [bool(x) for x in ctx.needs_input_grad[2:]]
        if g.shape[1] == 0:  # no points: zero gradients
            return (None, None) + tuple(torch.zeros_like(c) if need else None for c, need in zip(cores, needs))
        R = g.reshape(g.shape[1], g.shape[2]).contiguous()
        grads: List[Optional[torch.Tensor]] = [None] * k
        for n in range(k - 1, -1, -1):
            if needs[n]:
                perm, plan = ctx.plans[n]
                grads[n] = _hipops.gather_grad(Ls[n], R, perm, plan)
            if any(needs[:n]):  # R_{n-1}[p] = R_n[p] G_n[:, i_p, :]^T: the step on the core with its rank strides swapped
                R = _hip.gather_step(R, None, cores[n].permute(2, 1, 0), ctx.cols[n])
        return (None, None) + tuple(grads)


def point_eval(cores3: Sequence[torch.Tensor], cols: Sequence[torch.Tensor], cacheable: Optional[Sequence[bool]] = None) -> torch.Tensor:
    """Differentiable ``[1, P, r_k]`` core of the index-array block over device cores [r_n, I_n, r_{n+1}] (r_0 = 1)."""
    if cacheable is None:
        cacheable = [True] * len(cols)
    return _PointEval.apply(list(cols), list(cacheable), *cores3)


def wants_grad(t) -> bool:
    """Does ``t[key]`` have to be recorded by autograd on the device path?"""
    if not torch.is_grad_enabled():
        return False
    return any(x is not None and x.is_cuda and x.requires_grad for x in list(t.cores) + list(t.Us))


def getitem(t, key: list):
    """``t[key]`` for a processed key (one entry per mode) on a device train with parameters that require grad: index arrays on
    the first k >= 1 modes, slices on the rest."""
    from . import _hipops
    from .indexing import _index_column, _kind
    from .tensor import Tensor

    def refuse(what):
        raise NotImplementedError("tntorch_amd: {} is not differentiable on the device (supported: index arrays on the first "
                                  "modes of a non-batch TT / TT-Tucker train, slices on the rest); detach the cores or use CPU "
                                  "tensors".format(what))

    if t.batch:
        refuse("indexing a batched train")
    if any(c.dim() != 3 for c in t.cores):
        refuse("indexing CP cores")
    kinds = [_kind(x) for x in key]
    k = 0
    while k < len(kinds) and kinds[k] == "index":
        k += 1
    if k == 0 or any(kind != "slice" for kind in kinds[k:]):
        refuse("this key")
    if t.cores[0].shape[0] != 1:
        refuse("a leading boundary rank above 1")
    dev = t.cores[0].device
    _hipops._hip.lib()
    _hipops._hip.dtype_code(t.cores[0].dtype)
    cols = [_index_column(x, dev) for x in key[:k]]
    if any(len(c) != len(cols[0]) for c in cols):
        raise ValueError("Index arrays must have the same length")
    cacheable = [isinstance(x, torch.Tensor) and x.device == dev and x.dtype in (torch.int32, torch.int64) for x in key[:k]]
    block = []
    for n in range(k):
        c = t.cores[n]
        block.append(c if t.Us[n] is None else mode_mul(c[None], t.Us[n][None])[0])
    cores, Us = [point_eval(block, cols, cacheable)], [None]
    for n in range(k, len(t.cores)):
        if t.Us[n] is None:
            cores.append(t.cores[n][:, key[n], :])
            Us.append(None)
        else:
            cores.append(t.cores[n])
            Us.append(t.Us[n][key[n], :])
    return Tensor(cores, Us=Us)


# ---------------------------------------------------------------------------------------------- existing kernels, both directions
class _Gemm(torch.autograd.Function):
    """C[b] = A[b] @ B[b] (ttr_gemm); dA = g B^T, dB = A^T g."""

    @staticmethod
    def forward(ctx, A, B):
        from . import _hip

        ctx.save_for_backward(A, B)
        return _hip.gemm(A, B)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        from . import _hip

        A, B = ctx.saved_tensors
        dA = _hip.gemm(g, B, transB=True) if ctx.needs_input_grad[0] else None
        dB = _hip.gemm(A, g, transA=True) if ctx.needs_input_grad[1] else None
        return dA, dB


def gemm(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    return _Gemm.apply(A, B)


class _ModeMul(torch.autograd.Function):
    """[B, r0, S, r1] x_2 [B, a, S] -> [B, r0, a, r1]; the core's gradient is mode_mul(trans=True), the factor's one GEMM."""

    @staticmethod
    def forward(ctx, core4, M3):
        from . import _hipops

        ctx.save_for_backward(core4, M3)
        return _hipops.mode_mul(core4, M3)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        from . import _hip, _hipops

        core4, M3 = ctx.saved_tensors
        Bt, r0, S, r1 = core4.shape
        a = M3.shape[1]
        dcore = _hipops.mode_mul(g, M3, trans=True) if ctx.needs_input_grad[0] else None
        dM = None
        if ctx.needs_input_grad[1]:  # dM[b] = sum_{r0} g[b, r0] core[b, r0]^T
            gp = g.permute(0, 2, 1, 3).reshape(Bt, a, r0 * r1)
            cp = core4.permute(0, 2, 1, 3).reshape(Bt, S, r0 * r1)
            dM = _hip.gemm(gp, cp, transB=True)
        return dcore, dM


def mode_mul(core4: torch.Tensor, M3: torch.Tensor, trans: bool = False) -> torch.Tensor:
    if trans:
        raise NotImplementedError("tntorch_amd: mode_mul with a transposed factor is not differentiable on the device")
    return _ModeMul.apply(core4, M3)


class _DenseDist(torch.autograd.Function):
    """||a - b|| (ttr_gemm_axpby, ttr_norm); the gradients are +-(a - b) g / dist, zero where dist == 0."""

    @staticmethod
    def forward(ctx, a, b):
        from . import _hip

        n = a.numel()
        d = a.reshape(1, n, 1).clone()
        one = torch.ones((1, 1, 1), dtype=a.dtype, device=a.device)
        _hip.gemm_axpby(b.reshape(1, n, 1), one, d, -1.0, 1.0)
        dist = _hip.norm(d.reshape(1, -1))[0]
        ctx.save_for_backward(d, dist)
        ctx.shapes = (a.shape, b.shape)
        return dist

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        from . import _hip

        d, dist = ctx.saved_tensors
        s = torch.where(dist > 0, g / dist, torch.zeros_like(dist)).reshape(1, 1, 1)  # one element
        ga = _hip.gemm(d, s).reshape(ctx.shapes[0]) if ctx.needs_input_grad[0] else None
        gb = _hip.gemm(d, -s).reshape(ctx.shapes[1]) if ctx.needs_input_grad[1] else None
        return ga, gb


def dense_dist(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    if a.numel() != b.numel():
        raise ValueError("dist: the operands have {} and {} elements".format(a.numel(), b.numel()))
    return _DenseDist.apply(a, b)


# ---------------------------------------------------------------------------------------------- tt_multiply
class _TTMatvec(torch.autograd.Function):
    """y [b, cols] = x2d [b, rows] times the TT-matrix with the cores G_k [r_k, I_k, O_k, r_{k+1}] (r_0 = r_d = 1), through the
    three step functions of ``ops`` (``_hipops`` or ``_hostops``).  X_k [I_k, D_k, r_k] and Y_{k-1} [D_{k-1}, O_{k-1}, r_k] are
    the same memory, so a contiguous dX_k is dY_{k-1} as it lies: the backward chain copies nothing but ``dx``, transposed."""

    @staticmethod
    def forward(ctx, ops, x2d, *cores):
        needs = [bool(n) for n in ctx.needs_input_grad[2:]]
        X = x2d.t().contiguous()  # (grad mode is off in here: x2d and the cores still carry requires_grad, nothing is recorded)
        kept = []
        for G, need in zip(cores, needs):
            X = X.view(G.shape[1], -1, G.shape[0])
            kept.append(X if need else None)  # X_k is needed by dG_k only
            X = ops.ttm_step(X, G)
        ctx.ops = ops
        ctx.save_for_backward(*cores, *kept)
        return X.view(x2d.shape[0], -1)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        ops = ctx.ops
        d = len(ctx.saved_tensors) // 2
        cores, kept = ctx.saved_tensors[:d], ctx.saved_tensors[d:]
        need_x, needs = bool(ctx.needs_input_grad[1]), [bool(n) for n in ctx.needs_input_grad[2:]]
        grads: List[Optional[torch.Tensor]] = [None] * d
        b = g.shape[0]
        dY = g.contiguous()  # [b, cols] is dY_{d-1} [D_{d-1}, O_{d-1}, 1] as it lies
        for k in range(d - 1, -1, -1):
            G = cores[k]
            dY = dY.view(-1, G.shape[2], G.shape[3])
            if needs[k]:
                grads[k] = ops.ttm_grad_core(kept[k], dY)
            if not (need_x or any(needs[:k])):  # nothing earlier needs a gradient: the chain ends here
                break
            dY = ops.ttm_grad_input(dY, G)  # dX_k [I_k, D_k, r_k]: dY_{k-1}
        dx = dY.view(-1, b).t().contiguous() if need_x else None  # dX_0 is [rows, b]: the one transposed copy, as at entry
        return (None, dx) + tuple(grads)


def tt_matvec(cores: Sequence[torch.Tensor], x2d: torch.Tensor, ops) -> torch.Tensor:
    """Differentiable ``x2d [b, rows] @ M -> [b, cols]`` for TT-matrix cores [r_k, I_k, O_k, r_{k+1}] with boundary ranks 1.
    ``ops`` supplies ``ttm_step``, ``ttm_grad_input`` and ``ttm_grad_core``.  The forward is the chain of
    ``tt_matvec_chain`` (the same launches, the same bits); the backward launches one ``ttm_grad_core`` per core that requires
    grad and one ``ttm_grad_input`` per step with an operand before it that does."""
    return _TTMatvec.apply(ops, x2d, *cores)


# ---------------------------------------------------------------------------------------------- tt_embedding, tt_embedding_bag
class _TTRows(torch.autograd.Function):
    """out = pool(M[rows]) for the TT-matrix with the device cores G_k [r_k, I_k, O_k, r_{k+1}] (r_0 = r_d = 1): the chain of
    ``_hipops.tt_lookup_steps`` on the digit table, then -- with ``seg`` -- one ``ttr_segment_sum`` over the bags.  ``seg``
    (int64 [B + 1] or None: no pooling), ``weights`` ([P] or None), ``lengths`` ([B] in the dtype, the divisors of "mean", or
    None) and ``bad`` (a device bool: the offsets are invalid; or None) carry no gradient."""

    @staticmethod
    def forward(ctx, rows1d, seg, weights, lengths, bad, *cores):
        from . import _hipops, _hostops

        needs = [bool(n) for n in ctx.needs_input_grad[5:]]
        digits = _hostops.lookup_digits(cores, rows1d)
        # Z_k is needed by dG_k only; Z_1 = G_1[0, i_1] is read through the row map, never kept
        Y, flag, kept = _hipops.tt_lookup_steps(cores, digits, keep=needs)
        out = Y if seg is None else _hipops.segment_sum(Y, seg, w=weights)
        if lengths is not None:
            out = out / lengths[:, None]
        words = torch.stack([flag.reshape(()).to(torch.int32), (bad if bad is not None else flag.new_zeros(())).to(torch.int32)])
        oob, bad_offsets = words.tolist()  # the one host read of the call
        if bad_offsets:
            raise ValueError("tt_embedding_bag: the offsets must start at 0, not decrease and not pass the number of rows")
        if oob:
            raise IndexError("tt_lookup: a row index lies outside the matrix")
        ctx.d = len(cores)
        ctx.pooled = (seg is not None, weights is not None, lengths is not None)
        ctx.save_for_backward(*cores, *[z for z in kept if z is not None], digits,
                              *[t for t in (seg, weights, lengths) if t is not None])
        ctx.kept_at = [k for k, z in enumerate(kept) if z is not None]
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        from . import _hipops

        d, saved = ctx.d, list(ctx.saved_tensors)
        cores = saved[:d]
        kept = dict(zip(ctx.kept_at, saved[d:d + len(ctx.kept_at)]))
        digits = saved[d + len(ctx.kept_at)]
        rest = saved[d + len(ctx.kept_at) + 1:]
        seg = rest.pop(0) if ctx.pooled[0] else None
        weights = rest.pop(0) if ctx.pooled[1] else None
        lengths = rest.pop(0) if ctx.pooled[2] else None
        needs = [bool(n) for n in ctx.needs_input_grad[5:]]
        grads: List[Optional[torch.Tensor]] = [None] * d
        P, dev, dt = digits.shape[0], g.device, g.dtype
        # dY [P, cols]: the gradient of each sample's row (torch ops on the device; nothing is read back in here)
        if lengths is not None:
            g = g / lengths[:, None]
        if seg is not None:
            bag = torch.searchsorted(seg[1:].contiguous(), torch.arange(P, device=dev), right=True)
            g = g.index_select(0, bag)
            if weights is not None:
                g = g * weights[:, None]
        dY = g.contiguous()
        flag = torch.zeros(1, dtype=torch.int32, device=dev)  # (the forward validated the digits: it stays 0 and is not read)
        for k in range(d - 1, 0, -1):
            if not any(needs[:k + 1]):  # nothing from here down needs a gradient: the chain ends
                break
            G = cores[k].contiguous()
            R, I, O, S = G.shape
            col = digits[:, k]
            perm = torch.sort(col, stable=True).indices  # on the device; shared by the two launches of this step
            if needs[k]:
                X, xrow = (cores[0][0].contiguous(), digits[:, 0]) if k == 1 else (kept[k], None)
                grads[k] = _hipops.ttm_lookup_grad_core(X, xrow, dY, col, perm, flag,
                                                        torch.empty((R, I, O, S), dtype=dt, device=dev))
            if not any(needs[:k]):
                break
            dY = _hipops.ttm_lookup_grad_input(dY, G, col, perm, flag)  # dZ_{k-1} [P, D, R]: the next step's dY as it lies
        if needs[0]:  # dG_1[0, i] = the sum of dZ_1[p] over the samples with i_1 = i: the stable groups of the first digit
            I1 = cores[0].shape[1]
            srt = torch.sort(digits[:, 0], stable=True)
            seg0 = torch.searchsorted(srt.values, torch.arange(I1 + 1, device=dev))
            grads[0] = _hipops.segment_sum(dY.view(P, -1), seg0, perm=srt.indices).view(cores[0].shape)
        return (None, None, None, None, None) + tuple(grads)


def tt_rows(cores: Sequence[torch.Tensor], rows1d: torch.Tensor, seg: Optional[torch.Tensor] = None,
            weights: Optional[torch.Tensor] = None, lengths: Optional[torch.Tensor] = None,
            bad: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Differentiable rows ``rows1d`` [P] of the TT-matrix with the device cores G_k [r_k, I_k, O_k, r_{k+1}] -> [P, cols], or
    -- with ``seg`` (int64 [B + 1], the bounds of the bags) -- their sums over the bags, weighted by ``weights`` [P] and divided
    by ``lengths`` [B] -> [B, cols].  ``bad``: a device bool, checked (ValueError) in the one host read of the call, next to the
    out-of-range word (IndexError).

    The forward is the launches of ``tt_lookup_chain`` (the same bits) and one ``ttr_segment_sum`` for the bags.  It keeps the
    digit table and, for every core k >= 3 that requires grad, the state Z_{k-1} [P, O_1 .. O_{k-1}, r_{k-1}] that entered its
    step: THAT is the memory cost of training (the plain lookup keeps one state at a time); Z_1 is read from the first core.  The
    backward synchronises nothing: per step one stable ``torch.sort`` of the digit column on the device (no plan, no counts on
    the host), ``ttr_ttm_lookup_grad_core`` where the core requires grad and ``ttr_ttm_lookup_grad_input`` where an earlier one
    does, and one ``ttr_segment_sum`` over the groups of the first digit for the first core.  A frozen core costs no launch and
    gets no gradient.  No double backward, no gradient of ``weights``."""
    return _TTRows.apply(rows1d, seg, weights, lengths, bad, *cores)


# ---------------------------------------------------------------------------------------------- autodiff.py:10-121
def _parameters(tensors) -> list:
    from .tensor import Tensor

    params = []
    for t in tensors:
        if isinstance(t, Tensor):
            if t.batch:
                raise ValueError("Batched tensors are not supproted.")
            params += [c for c in t.cores if c.requires_grad]
            params += [U for U in t.Us if U is not None and U.requires_grad]
        elif t.requires_grad:
            params.append(t)
    return params


def optimize(tensors, loss_function, optimizer=torch.optim.Adam, tol=1e-4, max_iter=1e4, print_freq=500, verbose=True):
    """Iterative fitting (autodiff.py:10-101): ``tensors`` (one or several ``Tensor`` / ``torch.Tensor``) are passed to
    ``loss_function``, which returns a scalar or a tuple of scalars, and their cores and factors with ``requires_grad=True`` are
    updated in place by ``optimizer`` (a callable on the parameter list; default ``torch.optim.Adam``).

    It stops when the loss falls to ``tol`` or its relative improvement does (and the improvement is slowing down), or after
    ``max_iter`` iterations; progress is printed every ``print_freq`` iterations.  CPU and device trains; the total loss is read
    from the device once per iteration.  Batched tensors and a call without parameters raise ValueError."""
    if not isinstance(tensors, (list, tuple)):
        tensors = [tensors]
    params = _parameters(tensors)
    if not params:
        raise ValueError("There are no parameters to optimize. Did you forget a requires_grad=True somewhere?")
    opt = optimizer(params)
    width = len("{}".format(max_iter))

    def report(it, parts, total, end="\n"):
        line = "iter: {: <{}} | loss: ".format(it, width) + " + ".join("{:10.6f}".format(p.item()) for p in parts)
        if len(parts) > 1:
            line += " = {:10.4}".format(total)
        print(line + " | total time: {:9.4f}".format(time.time() - start), end=end)

    history: List[float] = []
    start = time.time()
    it, converged = 0, False
    while True:
        opt.zero_grad()
        parts = loss_function(*tensors)
        if not isinstance(parts, (tuple, list)):
            parts = [parts]
        total = sum(parts)
        total.backward(retain_graph=True)
        opt.step()
        history.append(float(total.detach()))  # the one read of the iteration
        if it >= 2 and tol is not None:
            cur, prev, before = history[-1], history[-2], history[-3]
            small = cur <= tol or (cur != 0 and (prev - cur) / cur <= tol)
            if small and prev - cur < before - prev:
                converged = True
                break
        if it == max_iter:
            break
        if verbose and it % print_freq == 0:
            report(it, parts, history[-1])
        it += 1
    if verbose:
        report(it, parts, history[-1], end="")
        print(" <- converged (tol={})".format(tol) if converged else " <- max_iter was reached: {}".format(max_iter))


def dof(t) -> int:
    """Degrees of freedom (autodiff.py:104-121): the number of elements of the cores and factors with ``requires_grad=True``."""
    nodes = list(t.cores) + [U for U in t.Us if U is not None]
    return sum(x.numel() for x in nodes if x.requires_grad)

"""TT-cross approximation (cross.py:138-530): a tensor train built from samples of a black-box function, or of a function of
existing tensor trains, taken on fibres chosen by maxvol.

Same signature, defaults, return values, ``info`` keys and random draws as the reference (``torch.randn`` for the initial cores,
``np.random.randint`` column blocks for the right index sets, ``np.random.choice`` for the validation set, the kickrank
``extra`` blocks), so a seeded call reproduces the reference's index sets.

CPU cores follow the reference's operator sequence (einsum, ``torch.linalg.qr``, maxvol, ``lstsq``; maxvol is the host mirror
of ``tntorch_amd.maxvol``).  Device cores run, per step of a sweep: the fibre evaluation ``ai,ibj,jc->abc`` as two ``ttr_gemm``,
the user's function, ``ttr_qr``, ``ttr_maxvol`` (whose fresh solve ``Q Q_I^-1`` is the new core: the reference's ``lstsq``),
and the interface update as one ``ttr_gather_step`` launch per input tensor.  Index sets stay on the device; a sweep reads one
value back to the host (validation error and invalid-value flag together).  Right interfaces are kept transposed (``[P, r]``)
on the device, so that every update is a row-gathered product.

``minimum``, ``argmin``, ``maximum`` and ``argmax`` (cross.py:12-109) run ``cross(..., _minimize=True)``: every evaluated fibre
block goes through Oseledets' map ``pi/2 - atan(f - best)``, so that maxvol steers the index sets towards small values, and the
best sample seen is carried along.  That is one ``minimize_step`` per block (``ttr_minimize_step`` on the device: one pass over
the block, the running best kept in device memory, nothing read back; its mirror on the CPU), and both maxvol calls become
``maxvol(Q, 1.05, 10)``, which is what the reference's ``rect_maxvol(Q, maxK=Q.shape[1])`` computes (it adds no rows).

Unlike the reference: the best value is the evaluated sample itself, not ``tan(pi/2 - y) + min`` (a round trip that loses
digits as ``|f - min|`` grows); the winning sample of a block is the first smallest ``f``, not the first largest transformed
value (the map can round distinct values together); a ``found`` flag replaces the ``info["min"] == 0`` sentinel, so a function
whose minimum is exactly 0 keeps it; a non-finite sample raises ``ValueError`` (the map sends ``+Inf`` to a finite value).  Batched
tensors, CP cores on the device and ranks above 128 on the device are refused as for ``cross``.

``cross_forward`` and a public ``rect_maxvol`` are out of scope.
"""

from __future__ import annotations

import logging
import sys
import time
from typing import Any, Callable, Sequence, Union

import numpy as np
import torch

__all__ = ["cross", "minimum", "argmin", "maximum", "argmax"]

MAX_DEVICE_RANK = 128  # ttr_maxvol's limit (r x r inverse in LDS): device cores take no larger bond


# ------------------------------------------------------------------------------------------------ host path (reference ops)
def _init_interfaces_host(tensors, rsets, N, device, dtype):
    """cross.py:115-135."""
    t_linterfaces, t_rinterfaces = [], []
    for t in tensors:
        linterfaces = [torch.ones(1, int(t.ranks_tt[0]), dtype=dtype).to(device)] + [None] * (N - 1)
        rinterfaces = [None] * (N - 1) + [torch.ones(int(t.ranks_tt[t.dim()]), 1, dtype=dtype).to(device)]
        for j in range(N - 1):
            M = torch.ones(t.cores[-1].shape[-1], len(rsets[j]), dtype=dtype).to(device)
            for n in range(N - 1, j, -1):
                if t.cores[n].dim() == 3:
                    M = torch.einsum("iaj,ja->ia", [t.cores[n][:, rsets[j][:, n - 1 - j], :].to(device), M])
                else:
                    M = torch.einsum("ai,ia->ia", [t.cores[n][rsets[j][:, n - 1 - j], :].to(device), M])
            rinterfaces[j] = M
        t_linterfaces.append(linterfaces)
        t_rinterfaces.append(rinterfaces)
    return t_linterfaces, t_rinterfaces


# ------------------------------------------------------------------------------------------------ device path (HIP kernels)
def _init_interfaces_dev(tensors, rsets, N, device, dtype):
    """cross.py:115-135 with gather steps; right interfaces transposed: ``rt[j]`` [P_j, r_{j+1}] = R_j^T."""
    from . import _hipops

    t_linterfaces, t_rinterfaces = [], []
    for t in tensors:
        linterfaces = [torch.ones(1, int(t.cores[0].shape[0]), dtype=dtype, device=device)] + [None] * (N - 1)
        rinterfaces = [None] * (N - 1) + [torch.ones(1, int(t.cores[-1].shape[-1]), dtype=dtype, device=device)]
        for j in range(N - 1):
            M = torch.ones(len(rsets[j]), int(t.cores[-1].shape[-1]), dtype=dtype, device=device)
            for n in range(N - 1, j, -1):
                M = _hipops.gather_step(M, None, t.cores[n].permute(2, 1, 0), rsets[j][:, n - 1 - j])
            rinterfaces[j] = M
        t_linterfaces.append(linterfaces)
        t_rinterfaces.append(rinterfaces)
    return t_linterfaces, t_rinterfaces


def _fibres_dev(L, core, Rt):
    """``einsum('ai,ibj,jc->abc', L, core, Rt^T)`` as two ttr_gemm -> flat [Ra * I * Rb]."""
    from . import _hip

    r0, I, r1 = core.shape
    T1 = _hip.gemm(L[None], core.reshape(1, r0, I * r1))  # [1, Ra, I * r1]
    V = _hip.gemm(T1.reshape(1, -1, r1), Rt[None], transB=True)  # [1, Ra * I, Rb]
    return V.reshape(-1)


def _chain_dev(cores, idx):
    """Values of a TT at P points given by one device index vector per mode: a chain of gather steps (no readback)."""
    from . import _hipops

    X = torch.ones(idx[0].shape[0], 1, dtype=cores[0].dtype, device=cores[0].device)
    for c, i in zip(cores, idx):
        X = _hipops.gather_step(X, None, c, i)
    return X[:, 0]


def _values_host(t, idx):
    """t[idx] for host trains with CP factors (indexing covers TT cores only): the product of the selected slices, summed over
    the last rank (the reference's CP-TT point evaluation)."""
    X = torch.ones(len(idx[0]), int(t.ranks_tt[0]), dtype=t.cores[0].dtype)
    for c, i in zip(t.cores, idx):
        X = torch.einsum("pa,apb->pb", X, c[:, i, :]) if c.dim() == 3 else X * c[i, :]
    return X.sum(dim=1)


def cross(
    function: Callable = lambda x: x,
    domain=None,
    tensors: Union[Any, Sequence[Any]] = None,
    function_arg: str = "vectors",
    ranks_tt: Union[int, Sequence[int]] = None,
    kickrank: int = 3,
    rmax: int = 100,
    eps: float = 1e-6,
    max_iter: int = 25,
    val_size: int = 1000,
    verbose: bool = True,
    return_info: bool = False,
    record_samples: bool = False,
    _minimize: bool = False,
    device: Any = None,
    suppress_warnings: bool = False,
    detach_evaluations: bool = False,
):
    """Cross-approximation of ``function`` over a ``domain`` (N vectors) or of a function of ``tensors`` (cross.py:138-530).

    :param function: gets N vectors of P elements (``function_arg='vectors'``) or a [P, N] matrix (``'matrix'``); returns P values
    :param domain: a list of N vectors (incompatible with ``tensors``)
    :param tensors: a :class:`Tensor` or list thereof, all of the same shape
    :param ranks_tt: int or N-1 ints; None: adaptive, starting at 1 and growing by ``kickrank`` per sweep up to ``rmax``
    :param eps: stop when the relative error on the validation set falls below this
    :param max_iter: maximal number of sweeps (left-to-right and back)
    :param val_size: size of the validation set
    :param return_info: also return a dictionary (``nsamples``, ``eval_time``, ``val_epss``, ``lsets``, ``rsets``, ``Rs``,
        ``left_locals``, ``total_time``, ``val_eps``, ...)
    :param record_samples: keep every sample position / value in ``info``
    :param device: PyTorch device (default: that of ``tensors``, or of ``domain``)
    :param suppress_warnings: hide the warning about insufficient accuracy
    :param detach_evaluations: detach the function's results from autograd

    :return: an N-dimensional TT :class:`Tensor` (and a dictionary, if ``return_info``)
    """
    from . import _hostops
    from .maxvol import maxvol
    from .tensor import Tensor
    from .tools import meshgrid

    if device is None and tensors is not None:
        device = (tensors[0] if isinstance(tensors, list) else tensors).cores[0].device
    if device is None and domain is not None:
        dom = domain[0] if hasattr(domain, "__len__") and len(domain) and hasattr(domain[0], "__len__") else domain
        if isinstance(dom, torch.Tensor):
            device = dom.device
    if verbose:
        print("cross device is", device)

    assert domain is not None or tensors is not None
    assert function_arg in ("vectors", "matrix")
    if function_arg == "matrix":

        def f(*args):
            return function(torch.cat([arg[:, None] for arg in args], dim=1))

    else:
        f = function

    if detach_evaluations:
        inner = f

        def f(*args):
            res = inner(*args)
            if hasattr(res, "__len__") and not isinstance(res, torch.Tensor):
                for i in range(len(res)):
                    if isinstance(res[i], torch.Tensor):
                        res[i] = res[i].detach()
            elif isinstance(res, torch.Tensor):
                res = res.detach()
            return res

    if tensors is None:
        tensors = meshgrid(domain)
    if not hasattr(tensors, "__len__"):
        tensors = [tensors]
    for t in tensors:
        if t.batch:
            raise ValueError("Batched tensors are not supported.")
    tensors = [t.decompress_tucker_factors(_clone=False) if any(U is not None for U in t.Us) else t for t in tensors]
    device = torch.device(device) if device is not None else tensors[0].cores[0].device
    if any(c.device != device for t in tensors for c in t.cores):
        tensors = [Tensor([c.to(device) for c in t.cores]) for t in tensors]
    on_dev = device.type != "cpu"
    dtype = tensors[0].cores[0].dtype
    if on_dev:
        from ._dispatch import ops_for

        ops_for(tensors[0].cores[0])  # the library and the dtype, checked up front
        if any(c.dim() != 3 for t in tensors for c in t.cores):
            raise NotImplementedError("cross: CP-format cores are not supported on the device")
        tensors = [Tensor([c.detach() for c in t.cores]) for t in tensors]
    Is = list(tensors[0].shape)
    N = len(Is)

    # Ranks, capped by the mode sizes (cross.py:267-280)
    if ranks_tt is None:
        ranks_tt = 1
    else:
        kickrank = None
    if not hasattr(ranks_tt, "__len__"):
        ranks_tt = [ranks_tt] * (N - 1)
    ranks_tt = [1] + list(ranks_tt) + [1]
    Rs = np.array(ranks_tt)
    for n in list(range(1, N)) + list(range(N - 1, -1, -1)):
        Rs[n] = min(Rs[n - 1] * Is[n - 1], Rs[n], Is[n] * Rs[n + 1])
    if on_dev and max(Rs) > MAX_DEVICE_RANK:  # before the function is first called
        raise NotImplementedError(
            "cross: ranks above {} are not supported on the device (capped ranks {})".format(MAX_DEVICE_RANK, Rs.tolist()))

    # Random draws in the reference's order: initial cores, right sets, validation set (cross.py:282-300)
    cores = [torch.randn(Rs[n], Is[n], Rs[n + 1]) for n in range(N)]
    lsets = [np.array([[0]])] + [None] * (N - 1)
    randint = np.hstack([np.random.randint(0, Is[n + 1], [max(Rs), 1]) for n in range(N - 1)] + [np.zeros([max(Rs), 1], dtype=int)])
    rsets = [randint[: Rs[n + 1], n:] for n in range(N - 1)] + [np.array([[0]])]
    Xs_val = [torch.as_tensor(np.random.choice(I, int(val_size))).to(device) for I in Is]

    if on_dev:
        from . import _hip, _hipops

        lsets = [torch.as_tensor(s, dtype=torch.int64, device=device) if s is not None else None for s in lsets]
        rsets = [torch.as_tensor(s, dtype=torch.int64, device=device) for s in rsets]
        init_interfaces = _init_interfaces_dev
        ys_val = f(*[_chain_dev(t.cores, Xs_val) for t in tensors])
    else:
        init_interfaces = _init_interfaces_host
        ys_val = f(*[t[Xs_val].torch() if all(c.dim() == 3 for c in t.cores) else _values_host(t, Xs_val) for t in tensors])
    t_linterfaces, t_rinterfaces = init_interfaces(tensors, rsets, N, device, dtype)
    if ys_val.dim() > 1:
        assert ys_val.dim() == 2
        assert ys_val.shape[1] == 1
        ys_val = ys_val[:, 0]
    assert len(ys_val) == val_size
    norm_ys_val = _hip.norm(ys_val.reshape(1, -1))[0] if on_dev else torch.norm(ys_val)

    if verbose:
        print("Cross-approximation over a {}D domain containing {:g} grid points:".format(N, tensors[0].numel()))
    start = time.time()
    converged = False

    info = {"nsamples": 0, "eval_time": 0, "val_epss": [], "min": 0, "argmin": None}
    if record_samples:
        info["sample_positions"] = torch.zeros(0, N).to(device)
        info["sample_values"] = torch.zeros(0).to(device)
    invalid_dev = [torch.zeros((), dtype=torch.bool, device=device)] if on_dev else None
    if _minimize:  # the running best sample, on the tensors' device: value, position, (found, invalid)
        minimize_step = _hipops.minimize_step if on_dev else _hostops.minimize_step
        min_best = torch.zeros(1, dtype=dtype, device=device)
        min_pos = torch.zeros(N, dtype=torch.int64, device=device)
        min_flags = torch.zeros(2, dtype=torch.int32, device=device)

    def evaluate_function(j):  # the function over Rs[j] x Is[j] x Rs[j+1] fibres (cross.py:321-394)
        Xs = []
        for k, t in enumerate(tensors):
            if on_dev:
                Xs.append(_fibres_dev(t_linterfaces[k][j], t.cores[j], t_rinterfaces[k][j]))
            elif t.cores[j].dim() == 3:
                Xs.append(torch.einsum("ai,ibj,jc->abc", [t_linterfaces[k][j], t.cores[j], t_rinterfaces[k][j]]).flatten())
            else:
                Xs.append(torch.einsum("ai,bi,ic->abc", [t_linterfaces[k][j], t.cores[j], t_rinterfaces[k][j]]).flatten())
        eval_start = time.time()
        evaluation = f(*Xs)
        if record_samples:
            info["sample_positions"] = torch.cat((info["sample_positions"], torch.cat([x[:, None] for x in Xs], dim=1)), dim=0)
            info["sample_values"] = torch.cat((info["sample_values"], evaluation))
        info["eval_time"] += time.time() - eval_start
        if evaluation.dim() == 2:
            evaluation = evaluation[:, 0]
        if on_dev and _minimize:  # ttr_minimize_step sets the invalid flag in the pass that transforms the block
            evaluation = evaluation.to(dtype).contiguous()
            minimize_step(evaluation, Rs[j], Is[j], Rs[j + 1], lsets[j], rsets[j], min_best, min_pos, min_flags)
        elif on_dev:  # checked at the end of the sweep, with the validation error (no readback here)
            invalid_dev[0] = invalid_dev[0] | ~torch.isfinite(evaluation).all()
        else:
            invalid = torch.nonzero(torch.isnan(evaluation) | torch.isinf(evaluation))
            if len(invalid) > 0:
                invalid = invalid[0].item()
                raise ValueError(
                    "Invalid return value for function {}: f({}) = {}".format(
                        function,
                        ", ".join("{:g}".format(x[invalid].detach().cpu().numpy()) for x in Xs),
                        f(*[x[invalid : invalid + 1][:, None] for x in Xs]).item(),
                    )
                )
            if _minimize:  # (on a copy: the function may have returned its argument, or a tensor autograd tracks)
                evaluation = evaluation.detach().to(dtype).clone()
                minimize_step(evaluation, Rs[j], Is[j], Rs[j + 1], torch.as_tensor(lsets[j], dtype=torch.int64),
                              torch.as_tensor(rsets[j], dtype=torch.int64), min_best, min_pos, min_flags)
        V = torch.reshape(evaluation, [Rs[j], Is[j], Rs[j + 1]])
        info["nsamples"] += V.numel()
        return V

    left_locals = []
    for i in range(max_iter):
        if verbose:
            print("iter: {: <{}}".format(i, len("{}".format(max_iter)) + 1), end="")
            sys.stdout.flush()
        left_locals = []

        # Left-to-right: QR + maxvol towards the right
        for j in range(N - 1):
            V = torch.reshape(evaluate_function(j), [-1, Rs[j + 1]])
            if on_dev:
                Q = _hipops.qr(V.detach()[None])[0][0]
                local, C = maxvol(Q, 1.05, 10) if _minimize else maxvol(Q)
                cores[j] = C.reshape(Rs[j], Is[j], Rs[j + 1])
                local_r, local_i = local // Is[j], local % Is[j]
                lsets[j + 1] = torch.cat([lsets[j][local_r, :], local_i[:, None]], dim=1)
                for k, t in enumerate(tensors):
                    t_linterfaces[k][j + 1] = _hipops.gather_step(t_linterfaces[k][j], local_r, t.cores[j], local_i)
            else:
                Q, _ = torch.linalg.qr(V)
                local, _ = maxvol(Q.detach(), 1.05, 10) if _minimize else maxvol(Q.detach())
                local = local.numpy()
                cores[j] = torch.reshape(torch.linalg.lstsq(Q[local, :].t(), Q.t()).solution.t(), [Rs[j], Is[j], Rs[j + 1]])
                local_r, local_i = np.unravel_index(local, [Rs[j], Is[j]])
                lsets[j + 1] = np.c_[lsets[j][local_r, :], local_i]
                for k, t in enumerate(tensors):
                    if t.cores[j].dim() == 3:
                        t_linterfaces[k][j + 1] = torch.einsum(
                            "ai,iaj->aj", [t_linterfaces[k][j][local_r, :], t.cores[j][:, local_i, :]])
                    else:
                        t_linterfaces[k][j + 1] = torch.einsum(
                            "ai,ai->ai", [t_linterfaces[k][j][local_r, :], t.cores[j][local_i, :]])
            left_locals.append(local)

        # Right-to-left: QR + maxvol towards the left
        for j in range(N - 1, 0, -1):
            V = torch.reshape(evaluate_function(j), [Rs[j], -1])
            if on_dev:
                Q = _hipops.qr(V.detach().t()[None])[0][0]
                local, C = maxvol(Q, 1.05, 10) if _minimize else maxvol(Q)
                cores[j] = C.t().contiguous().reshape(Rs[j], Is[j], Rs[j + 1])
                local_i, local_r = local // Rs[j + 1], local % Rs[j + 1]
                rsets[j - 1] = torch.cat([local_i[:, None], rsets[j][local_r, :]], dim=1)
                for k, t in enumerate(tensors):
                    t_rinterfaces[k][j - 1] = _hipops.gather_step(t_rinterfaces[k][j], local_r, t.cores[j].permute(2, 1, 0), local_i)
            else:
                Q, _ = torch.linalg.qr(V.t())
                local, _ = maxvol(Q.detach(), 1.05, 10) if _minimize else maxvol(Q.detach())
                local = local.numpy()
                cores[j] = torch.reshape(torch.linalg.lstsq(Q[local, :].t(), Q.t()).solution, [Rs[j], Is[j], Rs[j + 1]])
                local_i, local_r = np.unravel_index(local, [Is[j], Rs[j + 1]])
                rsets[j - 1] = np.c_[local_i, rsets[j][local_r, :]]
                for k, t in enumerate(tensors):
                    if t.cores[j].dim() == 3:
                        t_rinterfaces[k][j - 1] = torch.einsum(
                            "iaj,ja->ia", [t.cores[j][:, local_i, :], t_rinterfaces[k][j][:, local_r]])
                    else:
                        t_rinterfaces[k][j - 1] = torch.einsum(
                            "ai,ia->ia", [t.cores[j][local_i, :], t_rinterfaces[k][j][:, local_r]])

        # Leave the first core ready
        cores[0] = evaluate_function(0)

        # Validation error: the one readback of the sweep
        if on_dev:
            val_eps = _hip.norm((ys_val - _chain_dev(cores, Xs_val)).reshape(1, -1))[0] / norm_ys_val
            if _minimize:
                host = torch.stack([val_eps.double(), min_flags[1].double(), min_best[0].double()]).cpu()
            else:
                host = torch.stack([val_eps.double(), invalid_dev[0].double()]).cpu()
            if host[1].item():
                raise ValueError("Invalid return value for function {}: NaN or Inf among the samples of sweep {}".format(function, i))
            val_eps_host = host[0].item()
            best_host = host[2].item() if _minimize else None
        else:
            val_eps = torch.norm(ys_val - Tensor(cores)[Xs_val].torch()) / norm_ys_val
            val_eps_host = val_eps
            best_host = min_best[0].item() if _minimize else None
        info["val_epss"].append(val_eps)
        if val_eps_host < eps:
            converged = True
        if verbose:
            if _minimize:
                print("| best: {:.8g}".format(best_host), end="")
            else:
                print("| eps: {:.3e}".format(float(val_eps_host)), end="")
            print(" | time: {:8.4f} | largest rank: {:3d}".format(time.time() - start, max(Rs)), end="")
            if converged:
                print(" <- converged: eps < {}".format(eps))
            elif i == max_iter - 1:
                print(" <- max_iter was reached: {}".format(max_iter))
            else:
                print()
        if converged:
            break
        elif i < max_iter - 1 and kickrank is not None:  # Augment ranks (cross.py:481-497)
            newRs = Rs.copy()
            newRs[1:-1] = np.minimum(rmax, newRs[1:-1] + kickrank)
            for n in list(range(1, N)) + list(range(N - 1, 0, -1)):
                newRs[n] = min(newRs[n - 1] * Is[n - 1], newRs[n], Is[n] * newRs[n + 1])
            if on_dev and max(newRs) > MAX_DEVICE_RANK:
                raise NotImplementedError(
                    "cross: rank growth to {} exceeds the device limit of {} (lower rmax)".format(max(newRs), MAX_DEVICE_RANK))
            extra = np.hstack(
                [np.random.randint(0, Is[n + 1], [max(newRs), 1]) for n in range(N - 1)] + [np.zeros([max(newRs), 1], dtype=int)]
            )
            for n in range(N - 1):
                if newRs[n + 1] > Rs[n + 1]:
                    add = extra[: newRs[n + 1] - Rs[n + 1], n:]
                    if on_dev:
                        rsets[n] = torch.cat([rsets[n], torch.as_tensor(add, dtype=torch.int64, device=device)], dim=0)
                    else:
                        rsets[n] = np.vstack([rsets[n], add])
            Rs = newRs
            t_linterfaces, t_rinterfaces = init_interfaces(tensors, rsets, N, device, dtype)

    if _minimize:  # read once, after the last sweep: the position (the value stays where the tensors are)
        info["min"] = min_best[0].clone()
        info["argmin"] = tuple(int(x) for x in min_pos.tolist())

    if val_eps_host > eps and not _minimize and not suppress_warnings:
        logging.warning("eps={:g} (larger than {}) when cross-approximating {}".format(float(val_eps_host), eps, function))

    if verbose:
        print(
            "Did {} function evaluations, which took {:.4g}s ({:.4g} evals/s)".format(
                info["nsamples"], info["eval_time"], info["nsamples"] / max(info["eval_time"], 1e-30)
            )
        )
        print()

    ret = Tensor([c if isinstance(c, torch.Tensor) else torch.tensor(c) for c in cores])
    if return_info:
        def host(x):
            return x.cpu().numpy() if isinstance(x, torch.Tensor) else x

        info["lsets"] = [host(s) for s in lsets]
        info["rsets"] = [host(s) for s in rsets]
        info["Rs"] = Rs
        info["left_locals"] = [host(s) for s in left_locals]
        info["total_time"] = time.time() - start
        info["val_eps"] = val_eps
        return ret, info
    return ret


def _optimum(tensors, function, rmax, max_iter, verbose, kwargs):
    _, info = cross(**kwargs, tensors=tensors, function=function, rmax=rmax, max_iter=max_iter, verbose=verbose, return_info=True,
                    _minimize=True)
    return info


def minimum(tensors=None, function=lambda x: x, rmax=10, max_iter=10, verbose=False, **kwargs):
    """Estimate the minimal element of a tensor, or of a function of one or several tensors (cross.py:12-37), by
    cross-approximation of ``pi/2 - atan(f - best)``.

    :param tensors: a :class:`Tensor` or a list of them (or pass ``domain=`` among the keyword arguments)
    :param function: applied to the tensors' entries (default: identity)
    :param rmax: passed to :func:`cross`; lower is faster, higher is more thorough (default 10)
    :param max_iter: passed to :func:`cross` (default 10)
    :param verbose: default False
    :param kwargs: passed to :func:`cross`

    :return: a 0-dim tensor on the tensors' device, in their dtype: the smallest sample that was evaluated (the sample itself,
        unlike the reference's ``tan`` round trip)
    """
    return _optimum(tensors, function, rmax, max_iter, verbose, kwargs)["min"]


def argmin(tensors=None, function=lambda x: x, rmax=10, max_iter=10, verbose=False, **kwargs):
    """Estimate the position of the minimal element (cross.py:40-61); arguments as for :func:`minimum`.

    :return: a tuple of N Python ints
    """
    return _optimum(tensors, function, rmax, max_iter, verbose, kwargs)["argmin"]


def maximum(tensors=None, function=lambda x: x, rmax=10, max_iter=10, verbose=False, **kwargs):
    """Estimate the maximal element (cross.py:64-85): :func:`minimum` of the negated function, negated."""
    return -_optimum(tensors, lambda *x: -function(*x), rmax, max_iter, verbose, kwargs)["min"]


def argmax(tensors=None, function=lambda x: x, rmax=10, max_iter=10, verbose=False, **kwargs):
    """Estimate the position of the maximal element (cross.py:88-109): :func:`argmin` of the negated function."""
    return _optimum(tensors, lambda *x: -function(*x), rmax, max_iter, verbose, kwargs)["argmin"]

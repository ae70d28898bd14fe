"""``Tensor``: the tensor-train container behind which the MI355X sweeps sit.

Drop-in for the TT / TT-Tucker subset of ``tntorch.Tensor`` (tntorch/tensor.py:107-2287): same
constructor keywords, attributes (``cores``, ``Us``, ``batch``, ``idxs``) and methods on
the orthogonalisation / rounding path -- ``left_orthogonalize`` / ``right_orthogonalize`` /
``orthogonalize`` / ``factor_orthogonalize`` (tensor.py:1771-1909), ``round_tt`` (tensor.py:2008-2083),
``round_tucker`` (tensor.py:1911-2006), ``round`` (tensor.py:2085-2098), the dense
``ranks_tt=`` / ``ranks_tucker=`` / ``eps=`` constructors (tensor.py:401-408, 436-439) -- plus the thin
helpers the reference's tests use around them (``torch()``, ``clone()``, ``ranks_tt``, ``+``, scalar ``* /``).

Cores are ``[R_k, I_k, R_{k+1}]`` row-major tensors (``batch=True`` prepends ``B``); the
methods REBIND list entries and never write into the storage of the tensors they were
given (tensor.py:1818-1832, 2066-2083).  CPU cores run the host mirror, device cores run
the HIP kernels; Tucker factors ``Us[n]`` are ``[I_n, S_n]`` matrices (or ``None``); CP cores and the
other tensor-network formats of the reference are outside this package's scope and raise
``NotImplementedError``.
"""

from __future__ import annotations

from typing import Any, List, Optional, Sequence, Union

import numpy as np
import torch

from ._dispatch import ops_for

__all__ = ["Tensor"]


def _not_in_scope(what: str):
    raise NotImplementedError(
        f"tntorch_amd implements the TT orthogonalisation/rounding hot path only; {what} is out of scope "
        "(see DESIGN.md, 'Out of scope')"
    )


class Tensor(object):
    """Tensor train with the API of ``tntorch.Tensor`` on the rounding path."""

    def __init__(
        self,
        data: Union[torch.Tensor, np.ndarray, Sequence[torch.Tensor]],
        Us: Optional[Sequence[Any]] = None,
        idxs: Optional[Any] = None,
        device: Optional[Any] = None,
        requires_grad: Optional[bool] = None,
        ranks_cp: Optional[int] = None,
        ranks_tucker: Optional[Sequence[int]] = None,
        ranks_tt: Optional[Union[int, Sequence[int]]] = None,
        eps: Optional[float] = None,
        max_iter: Optional[int] = 25,
        tol: Optional[float] = 1e-4,
        verbose: Optional[bool] = False,
        batch: Optional[bool] = False,
        algorithm: Optional[str] = "svd",
    ):
        self.batch = bool(batch)
        nb = 1 if self.batch else 0
        dense_Us = None
        if isinstance(data, (list, tuple)):  # explicit cores (tensor.py:165-192)
            cores = list(data)
            if not all(isinstance(c, torch.Tensor) and nb + 2 <= c.dim() <= nb + 3 for c in cores):
                raise ValueError("All tensor cores must have 2 (for CP) or 3 (for TT) dimensions")
            for n in range(len(cores) - 1):  # tensor.py:172-189 (a 2-D core is a CP factor [I, R])
                nxt = cores[n + 1]
                if cores[n].shape[-1] != (nxt.shape[nb] if nxt.dim() == nb + 3 else nxt.shape[nb + 1]):
                    raise ValueError("Core ranks do not match")
            if device is not None:
                cores = [c.to(device) for c in cores]
            self.cores = cores
        else:
            if isinstance(data, np.ndarray):  # tensor.py:195-203
                data = torch.tensor(data, device=device)
            elif isinstance(data, torch.Tensor):
                data = data.to(device)
            else:
                raise ValueError(
                    "A tntorch.Tensor may be built either from a list of cores, one NumPy ndarray, or one PyTorch tensor"
                )
            if data.dim() == 0:
                data = data * torch.ones(1, device=data.device, dtype=data.dtype)
            if eps is not None and (ranks_tt is not None or ranks_tucker is not None):
                raise ValueError("Specify eps or ranks, but not both")
            if ranks_cp is not None:  # CP-ALS, tensor.py:210-400
                if ranks_tt is not None:
                    raise ValueError("ALS for CP-TT is not yet supported")
                assert not hasattr(ranks_cp, "__len__")
                ops = ops_for(data)
                if ranks_tucker is None:  # HOSVD-initialised ALS on the tensor itself (tensor.py:219-277)
                    self.cores, self.cp_errors = ops.cp_als(data, int(ranks_cp), max_iter, tol, verbose, batch=self.batch)
                else:  # CP on the Tucker core (tensor.py:278-300): Tucker-round first, ALS from a random start
                    X = data if self.batch else data[None]
                    N = X.dim() - 1
                    rtk = list(ranks_tucker) if hasattr(ranks_tucker, "__len__") else [ranks_tucker] * N
                    assert len(rtk) == N
                    c4, Us3 = ops.dense_tucker_tt(X, rtk, None, algorithm, self.batch)
                    core = ops.decompress(c4)  # the dense Tucker core [B, S_1..S_N] (tensor.py:1702-1715)
                    lead = [core.shape[0]] if self.batch else []
                    init = [torch.randn(lead + [sh, int(ranks_cp)], dtype=core.dtype, device=core.device) for sh in core.shape[1:]]
                    self.cores, self.cp_errors = ops.cp_als(core if self.batch else core[0], int(ranks_cp), max_iter, tol,
                                                            verbose, batch=self.batch, init=init)
                    dense_Us = [U if self.batch else U[0] for U in Us3]
            elif ranks_tucker is not None:
                self.cores, dense_Us = self._from_dense_tucker(data, ranks_tucker, ranks_tt, algorithm)
            else:
                self.cores = self._from_dense(data, ranks_tt, eps, algorithm)

        N = len(self.cores)
        if dense_Us is not None:
            Us = dense_Us
        if Us is None:
            Us = [None] * N
        Us = list(Us)
        if len(Us) != N:
            raise ValueError("There must be one Tucker factor (or None) per core")
        for n in range(N):  # tensor.py:410-424
            if Us[n] is None:
                continue
            if device is not None:
                Us[n] = Us[n].to(device)
            assert Us[n].dim() == nb + 2
            assert self.cores[n].shape[-2] == Us[n].shape[-1]
        self.Us = Us
        if requires_grad:
            for n in range(N):
                self.cores[n].requires_grad_()
                if self.Us[n] is not None:
                    self.Us[n].requires_grad_()
        self._idxs = idxs   # (built on first access: `idxs` below -- N arange launches per constructed tensor otherwise)
        if eps is not None:  # tensor.py:436-439
            if isinstance(data, (list, tuple)):
                if ranks_tt is not None or ranks_tucker is not None:
                    raise ValueError("Specify eps or ranks, but not both")
                self.round(eps, algorithm=algorithm)
            else:  # the TT stage of round() already ran inside _from_dense
                self._round_tucker_stage(data, eps, algorithm)

    # ------------------------------------------------------------------ dense -> TT
    def _from_dense(self, data: torch.Tensor, ranks_tt, eps, algorithm) -> List[torch.Tensor]:
        """tensor.py:401-408 / 436-439 for the TT format."""
        from . import _hostops

        X = data if self.batch else data[None]
        N = X.dim() - 1
        if ranks_tt is None and eps is None:  # exact, identity-padded TT (tensor.py:10-104)
            return self._denorm(_hostops.full_rank_tt(X))
        if N == 1:
            return self._denorm([X.reshape(X.shape[0], 1, X.shape[1], 1)])
        if eps is not None:
            # tensor.py:436-439 goes through round(): TT rounding here, then (``_round_tucker_stage``) Tucker
            # rounding with the remaining budget.
            rmax = [None] * (N - 1)
            e = eps
        else:
            rmax = list(ranks_tt) if hasattr(ranks_tt, "__len__") else [ranks_tt] * (N - 1)
            assert len(rmax) == N - 1
            e = 1e-14  # round_tt's default applies on the ctor path (tensor.py:408)
        ops = ops_for(X)
        return self._denorm(ops.dense_tt_svd(X, e, rmax, algorithm, self.batch))

    @classmethod
    def from_dense_consuming(cls, data: torch.Tensor, ranks_tt, algorithm: str = "svd") -> "Tensor":
        """EXTENSION (not in the reference): ``Tensor(data, ranks_tt=..., algorithm=...)`` for ONE dense device tensor whose
        storage may be OVERWRITTEN -- the first carry of the right-to-left TT-SVD (ranks_tt[-1] / I_N of the input) is written
        over the front of ``data`` instead of next to it, so a tensor that fills the device (BASELINE config C1: 64^6 fp32 =
        256 GiB of 288 GB) can be decomposed at all.  ``data`` holds garbage afterwards.  Same result as the constructor."""
        from . import _hipops

        if data.device.type != "cuda" or not data.is_contiguous() or data.dim() < 2:
            raise ValueError("from_dense_consuming needs a contiguous dense device tensor with >= 2 modes")
        N = data.dim()
        rmax = list(ranks_tt) if hasattr(ranks_tt, "__len__") else [ranks_tt] * (N - 1)
        assert len(rmax) == N - 1
        if data.shape[-1] > 64:
            # the in-place carry exists for the fused tall kernels (<= 64 columns).  A longer last mode completes through the
            # ordinary constructor path -- the behaviour of rounds 1 - 4 -- with the first carry NEXT to the input (peak memory
            # input x (1 + ranks_tt[-1] / I_N)); the caller is told, since memory is what this entry exists for
            import warnings

            warnings.warn("from_dense_consuming: last mode > 64, the first carry is written next to the input instead of over it "
                          f"(+ {rmax[-1]} / {data.shape[-1]} of the input's bytes)", RuntimeWarning, stacklevel=2)
            cores = _hipops.dense_tt_svd(data[None], 1e-14, rmax, algorithm, False)
            return cls([c[0] for c in cores])
        cores = _hipops.dense_tt_svd(data[None], 1e-14, rmax, algorithm, False, consume_input=True)
        return cls([c[0] for c in cores])

    def _from_dense_tucker(self, data: torch.Tensor, ranks_tucker, ranks_tt, algorithm):
        """tensor.py:401-408 with ``ranks_tucker`` (and optionally ``ranks_tt``)."""
        X = data if self.batch else data[None]
        N = X.dim() - 1
        rtk = list(ranks_tucker) if hasattr(ranks_tucker, "__len__") else [ranks_tucker] * N
        assert len(rtk) == N
        rtt = None
        if ranks_tt is not None:
            rtt = list(ranks_tt) if hasattr(ranks_tt, "__len__") else [ranks_tt] * (N - 1)
            assert len(rtt) == N - 1
        c, Us = ops_for(X).dense_tucker_tt(X, rtk, rtt, algorithm, self.batch)
        return self._denorm(c), [U if self.batch else U[0] for U in Us]

    def _round_tucker_stage(self, data: torch.Tensor, eps: float, algorithm):
        """Second half of ``round(eps)`` for the ``eps=`` constructor (tensor.py:2094-2098): the error reached
        by the TT stage is measured against the dense input itself."""
        from . import _hostops
        from .metrics import relative_error

        if self.dim() == 1:
            return
        if data.device.type == "cpu":  # exactly the reference: TT-vs-TT error against the full-rank train
            X = data if self.batch else data[None]
            reached = float(relative_error(Tensor(self._denorm(_hostops.full_rank_tt(X)), batch=self.batch), self))
        else:
            reached = float(relative_error(data, self))
        if reached < eps:
            self.round_tucker((1 + eps) / (1 + reached) - 1, algorithm=algorithm)

    # ------------------------------------------------------------------ layout helpers
    def _norm4(self, grad: bool = False) -> List[torch.Tensor]:
        """Cores as [B, r0, I, r1] views (B = 1 for non-batch tensors); CP factors [I, R] become TT cores whose
        slices are diagonal (tensor.py:1717-1769: first [1, I, R], last [R, I, 1], middle [R, I, R]).  ``grad``: the caller
        differentiates what it does with them (autodiff.py); everyone else is refused device parameters that require grad."""
        if not grad and any(x is not None and x.is_cuda and x.requires_grad for x in list(self.cores) + list(self.Us)):
            raise NotImplementedError(
                "tntorch_amd: the HIP kernels are not differentiable (autograd would silently see constants); "
                "detach the cores or run the rounding on CPU tensors")
        cs = list(self.cores) if self.batch else [c[None] for c in self.cores]
        N = len(cs)
        out = []
        for n, c in enumerate(cs):
            if c.dim() == 4:
                out.append(c)
            elif n == 0:
                out.append(c[:, None])
            elif n == N - 1:
                out.append(c.transpose(-1, -2)[..., None])
            else:
                Bt, I, R = c.shape
                core = c.new_zeros((Bt, R, I, R))
                idx = torch.arange(R, device=c.device)
                core[:, idx, :, idx] = c.permute(2, 0, 1)
                out.append(core)
        return out

    def _denorm(self, cores4: Sequence[torch.Tensor]) -> List[torch.Tensor]:
        return list(cores4) if self.batch else [c[0] for c in cores4]

    def _norm_us(self) -> List[Optional[torch.Tensor]]:
        """Factors as [B, I, S] (B = 1 for non-batch tensors)."""
        return [U if (U is None or self.batch) else U[None] for U in self.Us]

    def _denorm_us(self, Us3) -> List[Optional[torch.Tensor]]:
        return [U if (U is None or self.batch) else U[0] for U in Us3]

    def _has_factors(self) -> bool:
        return any(U is not None for U in self.Us)

    def _absorbed4(self, grad: bool = False) -> List[torch.Tensor]:
        """Cores [B, r0, I, r1] with the Tucker factors contracted in (``grad``: as for ``_norm4``; ``mode_mul`` is differentiable)."""
        c = self._norm4(grad)
        if not self._has_factors():
            return c
        return ops_for(c[0], grad).absorb_factors(c, self._norm_us())

    # ------------------------------------------------------------------ properties (tensor.py:836-919)
    @property
    def idxs(self):
        """tensor.py:433-435: one index vector per mode (identity indexing unless given to the constructor)."""
        if self._idxs is None:
            self._idxs = [torch.arange(sh, device=self.cores[0].device) for sh in self.shape]
        return self._idxs

    @idxs.setter
    def idxs(self, value):
        self._idxs = value

    @property
    def shape(self):
        shape = []
        if self.batch:
            shape.append(len(self.cores[0]))
        for c, U in zip(self.cores, self.Us):
            shape.append(c.shape[-2] if U is None else U.shape[-2])  # tensor.py:836-859
        return torch.Size(shape)

    def size(self):
        return self.shape

    def b(self):
        if not self.batch:
            raise ValueError
        return self.cores[0].shape[0]

    def dim(self):
        return len(self.cores)

    @property
    def ranks_tt(self):
        """tensor.py:861-883: CPU int64 tensor ``[R_0, R_1, ..., R_N]``."""
        nb = 1 if self.batch else 0
        c0 = self.cores[0]
        first = c0.shape[nb + 1] if c0.dim() == nb + 2 else c0.shape[nb]  # CP factor: R (tensor.py:878-881)
        return torch.tensor([first] + [c.shape[-1] for c in self.cores])

    @ranks_tt.setter
    def ranks_tt(self, value):
        self.round_tt(rmax=value)

    @property
    def ranks_tucker(self):
        return torch.tensor([c.shape[-2] for c in self.cores])

    def numel(self):
        return torch.round(torch.prod(torch.tensor(self.shape).double()))

    def numcoef(self):
        return sum(c.numel() for c in self.cores) + sum(U.numel() for U in self.Us if U is not None)

    def __repr__(self):
        fmt = "{}D TT tensor (batch)" if self.batch else "{}D TT tensor"
        return fmt.format(self.dim()) + ": shape {}, TT ranks {}, Tucker ranks {}, device {}, dtype {}".format(
            list(self.shape), self.ranks_tt.tolist(), self.ranks_tucker.tolist(), self.cores[0].device,
            self.cores[0].dtype
        )

    # ------------------------------------------------------------------ copies / conversion
    def clone(self):
        """tensor.py:2213-2229."""
        Us = [None if U is None else U.clone() for U in self.Us]
        return Tensor([c.clone() for c in self.cores], Us=Us, idxs=self._idxs, batch=self.batch)

    def to(self, device):
        """tensor.py:1689-1700 (in place, returns self)."""
        self.cores = [c.to(device) for c in self.cores]
        self.Us = [None if U is None else U.to(device) for U in self.Us]
        if self._idxs is not None:   # tensor.py:1703-1704 (lazily built here: only when they exist)
            self._idxs = [i.to(device) if torch.is_tensor(i) else i for i in self._idxs]
        return self

    def torch(self):
        """Decompress into a dense torch tensor (tensor.py:1639-1687, TT / TT-Tucker)."""
        grad = (not self.batch) and all(x.dim() == 3 for x in self.cores)  # differentiable on the device: non-batch TT / TT-Tucker
        c = self._absorbed4(grad)
        out = ops_for(c[0], grad).decompress(c)  # device tensors: chain of MFMA GEMMs (ttr_gemm)
        return out if self.batch else out[0]

    def numpy(self):
        return self.torch().detach().cpu().numpy()

    def decompress_tucker_factors(self, dim="all", _clone=True):
        """Contract Tucker factors into their cores (tensor.py:1576-1637): returns a tensor without factors along ``dim``
        (an int, a list, or ``'all'``).  ``_clone=False`` rebinds this tensor's cores instead of copying the others."""
        if isinstance(dim, str) and dim == "all":
            dims = list(range(self.dim()))
        elif hasattr(dim, "__len__"):
            dims = list(dim)
        else:
            dims = [dim]
        c4, Us3 = self._norm4(), self._norm_us()
        cores, Us = [], []
        for n in range(self.dim()):
            if n in dims and self.Us[n] is not None:
                cores.append(ops_for(c4[n]).mode_mul(c4[n], Us3[n]))
                Us.append(None)
            else:
                cores.append(c4[n].clone() if _clone else c4[n])
                Us.append(None if self.Us[n] is None else (self.Us[n].clone() if _clone else self.Us[n]))
        return Tensor(self._denorm(cores), Us=Us, idxs=self._idxs, batch=self.batch)

    # ------------------------------------------------------------------ indexing (tensor.py:1019-1434)
    def __getitem__(self, key):
        """NumPy-style indexing: ints, slices, ``None``, one ``Ellipsis`` and index arrays (lists, tuples, arrays, integer
        tensors; a 2-D ``[P, N]`` array is N columns).  Index arrays must be contiguous in the key and of equal length P; they
        become one ``[r_a, P, r_b]`` core.  An all-int key returns a 0-d tensor, every other key a ``Tensor``."""
        from .indexing import getitem

        return getitem(self, key)

    def __setitem__(self, key, value):
        _not_in_scope("assignment into a tensor train (__setitem__)")

    # ------------------------------------------------------------------ arithmetic used around the hot path
    def _scalar_like(self, value):
        c0 = self.cores[0]
        lead = (c0.shape[0],) if self.batch else ()
        cores = [torch.ones(lead + (1, c.shape[-2], 1), dtype=c0.dtype, device=c0.device) for c in self.cores]
        cores[0] = ops_for(cores[0]).scale(cores[0], value)
        return Tensor(cores, batch=self.batch)

    def __add__(self, other):
        """TT + TT: block-diagonal core concatenation, ranks add (tensor.py:445-668)."""
        if not isinstance(other, Tensor):
            other = self._scalar_like(other)
        if self.batch != other.batch:
            raise ValueError("Tensors with the same batch mode are supported")
        if self.shape != other.shape:
            raise ValueError("tntorch_amd: + requires equal shapes (broadcasting is out of scope)")
        N = self.dim()
        # Tucker factors are contracted into the cores first (the reference concatenates them instead,
        # tensor.py:445-668: same tensor, different -- equally redundant -- representation)
        ca, cb = self._denorm(self._absorbed4()), other._denorm(other._absorbed4())
        if N == 1:
            return Tensor([ca[0] + cb[0]], batch=self.batch)
        cores = []
        for n in range(N):
            a, b = ca[n], cb[n]
            if n == 0:
                cores.append(torch.cat([a, b], dim=-1))
            elif n == N - 1:
                cores.append(torch.cat([a, b], dim=-3))
            else:
                za = a.new_zeros(a.shape[:-1] + (b.shape[-1],))
                zb = b.new_zeros(b.shape[:-1] + (a.shape[-1],))
                cores.append(torch.cat([torch.cat([a, za], dim=-1), torch.cat([zb, b], dim=-1)], dim=-3))
        return Tensor(cores, batch=self.batch)

    def __radd__(self, other):
        return self + other

    def __neg__(self):
        return self * (-1)

    def __sub__(self, other):
        return self + (other * (-1) if isinstance(other, Tensor) else -other)

    def __rsub__(self, other):
        return (self * (-1)) + other

    def __mul__(self, other):
        if isinstance(other, Tensor):  # element-wise product: slice-wise Kronecker product of the cores
            if self.batch != other.batch:
                raise ValueError("Tensors with the same batch mode are supported")
            if self.shape != other.shape:
                raise ValueError("tntorch_amd: * requires equal shapes (broadcasting is out of scope)")
            ca, cb = self._absorbed4(), other._absorbed4()
            ops = ops_for(ca[0])
            return Tensor(self._denorm([ops.core_kron(a, b) for a, b in zip(ca, cb)]), batch=self.batch)
        cores = [c.clone() for c in self.cores]
        cores[0] = ops_for(cores[0]).scale(cores[0], other)
        return Tensor(cores, Us=[None if U is None else U.clone() for U in self.Us], batch=self.batch)

    def __rmul__(self, other):
        return self * other

    def __truediv__(self, other):
        if isinstance(other, Tensor):
            _not_in_scope("the quotient of two tensor trains")
        return self * (1.0 / other)

    # ------------------------------------------------------------------ Boolean logic (tensor.py:809-822)
    def __invert__(self):
        return 1 - self

    def __and__(self, other):
        return self * other

    def __or__(self, other):
        return self + other - self * other

    def __xor__(self, other):
        return self + other - 2 * self * other

    # ------------------------------------------------------------------ orthogonalisation (tensor.py:1771-1909)
    def left_orthogonalize(self, mu: int):
        """Make core ``mu`` left-orthogonal, push ``R`` into core ``mu+1`` (tensor.py:1800-1833)."""
        assert 0 <= mu < self.dim() - 1
        c, Us = self._norm4(), self._norm_us()
        R = ops_for(c[mu]).left_orthogonalize(c, mu, Us)
        self.cores, self.Us = self._denorm(c), self._denorm_us(Us)
        return R if self.batch else R[0]

    def right_orthogonalize(self, mu: int):
        """Make core ``mu`` right-orthogonal, push ``L`` into core ``mu-1`` (tensor.py:1835-1879)."""
        assert 1 <= mu < self.dim()
        c, Us = self._norm4(), self._norm_us()
        L = ops_for(c[mu]).right_orthogonalize(c, mu, Us)
        self.cores, self.Us = self._denorm(c), self._denorm_us(Us)
        return L if self.batch else L[0]

    def factor_orthogonalize(self, mu: int):
        """Push the non-orthogonal part of factor ``mu`` into its core (tensor.py:1771-1798)."""
        c, Us = self._norm4(), self._norm_us()
        ops_for(c[mu]).factor_orthogonalize(c, Us, mu)
        self.cores, self.Us = self._denorm(c), self._denorm_us(Us)

    def orthogonalize(self, mu: int):
        """Make the train ``mu``-orthogonal; returns the last ``R, L`` (tensor.py:1881-1909)."""
        if mu < 0:
            mu += self.dim()
        dev = self.cores[0].device
        one = (self.cores[0].shape[0], 1, 1) if self.batch else (1, 1)
        L = torch.ones(one, device=dev, dtype=self.cores[0].dtype)
        R = torch.ones(one, device=dev, dtype=self.cores[0].dtype)
        for i in range(mu):
            R = self.left_orthogonalize(i)
        for i in range(self.dim() - 1, mu, -1):
            L = self.right_orthogonalize(i)
        return R, L

    # ------------------------------------------------------------------ rounding (tensor.py:2008-2098)
    def round_tt(
        self,
        eps: float = 1e-14,
        rmax: Optional[Union[int, Sequence[int]]] = None,
        algorithm: Optional[str] = "svd",
        verbose: Optional[bool] = False,
    ):
        """Recompress in place by reducing the TT ranks (tensor.py:2008-2083).

        ``eps``: relative error bound (ignored when ``batch=True``, tensor.py:2036-2037);
        ``rmax``: rank cap (int or one per bond); ``algorithm``: ``'svd'`` or ``'eig'``.
        """
        N = self.dim()
        if not hasattr(rmax, "__len__"):
            rmax = [rmax] * (N - 1)
        assert len(rmax) == N - 1
        assert algorithm in ("svd", "eig")
        for r in rmax:
            assert r is None or r >= 1
        if N == 1:
            return
        c, Us = self._norm4(), self._norm_us()
        ops = ops_for(c[0])
        ops.VERBOSE = bool(verbose)   # the reference's lines: "Orthogonalization time:", then per bond those of truncated_svd
        try:
            out = ops.round_tt(c, eps, list(rmax), algorithm, self.batch, Us if self._has_factors() else None)
        finally:
            ops.VERBOSE = False
        self.Us = self._denorm_us(Us)
        self.cores = self._denorm(out)

    @staticmethod
    def _round_of_sum(a: "Tensor", b: "Tensor", eps=1e-14, rmax=None, algorithm="svd"):
        """``round(a + b)`` (tensor.py:445-668 followed by tensor.py:2085-2098) for two pure TT tensors on the device
        without materialising the block-diagonal cores of the sum: the L2R sweep reads the two addends' cores directly
        (``ttr_qr_factor_pushed_sum``), and the error the TT stage reached is taken from inner products with the
        addends, <a+b, a+b> = <a,a> + 2<a,b> + <b,b>.  Returns None when the fusion does not apply (the caller then
        takes the generic path)."""
        from . import _hipops
        from .metrics import dot

        if not (isinstance(a, Tensor) and isinstance(b, Tensor)) or a.batch != b.batch or a.shape != b.shape:
            return None
        if a._has_factors() or b._has_factors() or a.dim() < 3:
            return None
        ca, cb = a._norm4(), b._norm4()
        if not (ca[0].is_cuda and cb[0].is_cuda and ca[0].dtype == cb[0].dtype):
            return None
        N = a.dim()
        rm = list(rmax) if hasattr(rmax, "__len__") else [rmax] * (N - 1)
        out = ops_for(ca[0]).round_tt(_hipops.sum_cores(ca, cb), eps, rm, algorithm, a.batch, None)
        res = Tensor(a._denorm(out), batch=a.batch)
        # second half of round(): Tucker stage with the remaining budget and the same kwargs Tensor.round passes on (rmax
        # included).  Batch tensors: the reference's round() cannot evaluate `reached` on a batch at all (relative_error ->
        # dot raises, metrics.py:28-116), and neither can this package's generic path; the fused sum is an extension there and,
        # like round_tt in batch mode (tensor.py:2036-2037), ignores eps: TT stage only.
        if not a.batch and eps > 0:
            gg = dot(a, a) + 2 * dot(a, b) + dot(b, b)
            err2 = (gg + dot(res, res) - 2 * (dot(a, res) + dot(b, res))).clamp(0)
            reached = float(torch.sqrt(err2) / torch.sqrt(gg.clamp(0)))
            if reached < eps:
                res.round_tucker((1 + eps) / (1 + reached) - 1, rmax=rmax, algorithm=algorithm)
        return res

    def round_tucker(
        self,
        eps: float = 1e-14,
        rmax: Optional[Union[int, Sequence[int]]] = None,
        dim: Optional[Union[Sequence[int], str]] = "all",
        algorithm: Optional[str] = "svd",
    ):
        """Recompress in place by reducing the Tucker ranks (tensor.py:1911-2006).

        As in the reference every mode is processed; ``dim`` only sets how the error budget is split
        (``eps / sqrt(len(dim))`` per mode, tensor.py:1936-1939, 1991)."""
        N = self.dim()
        if not hasattr(rmax, "__len__"):
            rmax = [rmax] * N
        assert len(rmax) == N
        assert algorithm in ("svd", "eig")
        if dim == "all":
            dim = range(N)
        if not hasattr(dim, "__len__"):
            dim = [dim] * N
        c, Us = self._norm4(), self._norm_us()
        c, Us = ops_for(c[0]).round_tucker(c, Us, eps, list(rmax), len(dim), algorithm, self.batch)
        self.cores, self.Us = self._denorm(c), self._denorm_us(Us)

    def round(self, eps: float = 1e-14, **kwargs):
        """General recompression (tensor.py:2085-2098): TT ranks first, then Tucker rounding with the
        remaining error budget."""
        from .metrics import relative_error

        copy = self.clone()
        self.round_tt(eps, **kwargs)
        reached = relative_error(copy, self)
        if reached < eps:
            self.round_tucker((1 + eps) / (1 + float(reached)) - 1, **kwargs)

    # ------------------------------------------------------------------ convenience "methods" (tensor.py:2125-2137)
    def var(self, **kwargs):
        """See :func:`metrics.var`."""
        from .metrics import var

        return var(self, **kwargs)

    def std(self, **kwargs):
        """See :func:`metrics.std`."""
        from .metrics import std

        return std(self, **kwargs)

"""``TTMatrix`` / ``CPMatrix``: a matrix stored as a tensor train of ``[r, i_k, o_k, r']`` cores or as CP factors
``[i_k, o_k, R]``, and its product with a batch of vectors, ``tt_multiply`` / ``cp_multiply`` (``tntorch/matrix.py``; SURVEY
8f-4: the consumer that sits directly on the dense TT-SVD; DESIGN section 24 for the products).

A matrix ``M`` of shape ``prod(input_dims) x prod(output_dims)`` is reshaped to ``i_0 x ... x i_{d-1} x o_0 x ... x o_{d-1}``,
its axes interleaved to ``(i_0 o_0) x ... x (i_{d-1} o_{d-1})``, decomposed by ``Tensor(..., ranks_tt=ranks)`` -- on device
tensors the streaming right-to-left TT-SVD kernels -- and every core ``[r, i_k o_k, r']`` is viewed as ``[r, i_k, o_k, r']``.
``torch()`` contracts the train (a chain of MFMA GEMMs on the device) and undoes the interleaving.

``tt_multiply(ttm, x)`` is ``x.reshape(b, rows) @ ttm.torch()`` without the dense matrix: ``d`` steps, each a GEMM over the pair
(input index, rank) of one core.  With the reference's index order the row-major output of a step is the input of the next one
as it lies, so on the device the chain is ``d`` launches of ``ttr_ttm_step`` and one transposed copy of ``x`` at entry;
``cp_multiply`` is the same chain with the rank carried (``ttr_cpm_step``) and summed at the end (``ttr_mode_reduce``).
Unlike the reference, both check their operands and raise ``ValueError`` (the reference fails an ``assert`` or inside einsum).
``tt_multiply`` is differentiable on the device in the cores and in the tensor (``autodiff.tt_matvec``: two fused backward
kernels per step, ``ttr_ttm_grad_core`` and ``ttr_ttm_grad_input``); ``cp_multiply`` is not, and says so.
Not here: ``determinant`` / ``slog_determinant`` / ``inv`` / ``cholesky`` (the reference's own guard raises for every square
matrix, so none of them can run there), the transposed product as a public call and autograd through ``cp_multiply`` on the
device.
"""

from __future__ import annotations

from typing import List, Optional, Sequence, Union

import torch

from ._dispatch import ops_for
from .tensor import Tensor

__all__ = ["TTMatrix", "CPMatrix", "tt_multiply", "cp_multiply"]


class TTMatrix:
    """Same constructor contract as ``tntorch.TTMatrix`` (matrix.py:23-111)."""

    def __init__(self, t: Union[torch.Tensor, Sequence[torch.Tensor]], ranks: Optional[List[int]], input_dims: Sequence[int],
                 output_dims: Sequence[int]):
        assert len(input_dims) == len(output_dims)
        assert len(input_dims) > 0
        self.input_dims = torch.tensor(list(input_dims))
        self.output_dims = torch.tensor(list(output_dims))
        self.d = len(input_dims)
        idims, odims = [int(x) for x in input_dims], [int(x) for x in output_dims]

        if isinstance(t, (list, tuple)):  # pre-processed cores (matrix.py:48-57)
            core_dims = len(t[0].shape)
            assert core_dims in [4, 5]
            self.batch = core_dims == 5  # b x r_{i-1} x input_i x output_i x r_i
            self.cores = list(t)
            self.ranks = torch.tensor([c.shape[-1] for c in t[:-1]])
            return

        assert isinstance(ranks, list) and len(ranks) == self.d - 1
        M = t
        assert len(M.shape) in [2, 3]
        self.batch = len(M.shape) == 3
        nb = 1 if self.batch else 0
        rows, cols = 1, 1
        for a, b in zip(idims, odims):
            rows, cols = rows * a, cols * b
        assert rows == M.shape[-2]
        assert cols == M.shape[-1]

        lead = [M.shape[0]] if self.batch else []
        tensor = M.reshape(lead + idims + odims)
        # i_0 .. i_{d-1} o_0 .. o_{d-1}  ->  i_0 o_0 i_1 o_1 ...  (matrix.py:69-92); a layout copy
        perm = list(range(nb)) + [nb + k + off for k in range(self.d) for off in (0, self.d)]
        tensor = tensor.permute(perm).reshape(lead + [idims[k] * odims[k] for k in range(self.d)])
        if not tensor.is_contiguous():
            tensor = tensor.contiguous()
        tt = Tensor(tensor, ranks_tt=ranks, batch=self.batch)
        self.ranks = tt.ranks_tt[1:-1]
        self.cores = [
            c.reshape((list(c.shape[:nb + 1])) + [idims[k], odims[k], c.shape[-1]]) for k, c in enumerate(tt.cores)
        ]

    # ------------------------------------------------------------------ conversions (matrix.py:113-158)
    def flatten(self) -> Tensor:
        """The train with every core's input and output mode merged: a ``Tensor`` of shape ``(i_k o_k)_k`` (matrix.py:177-201)."""
        nb = 1 if self.batch else 0
        return Tensor([c.reshape(list(c.shape[:nb + 1]) + [c.shape[nb + 1] * c.shape[nb + 2], c.shape[-1]]) for c in self.cores],
                      batch=self.batch)

    def torch(self) -> torch.Tensor:
        """Decompress into a dense ``rows x cols`` matrix (batch: ``b x rows x cols``)."""
        idims, odims = self.input_dims.tolist(), self.output_dims.tolist()
        nb = 1 if self.batch else 0
        dense = self.flatten().torch()
        lead = [dense.shape[0]] if self.batch else []
        shape = [x for k in range(self.d) for x in (idims[k], odims[k])]
        dense = dense.reshape(lead + shape)
        perm = list(range(nb)) + [nb + 2 * k for k in range(self.d)] + [nb + 2 * k + 1 for k in range(self.d)]
        rows, cols = int(torch.prod(self.input_dims)), int(torch.prod(self.output_dims))
        return dense.permute(perm).reshape(lead + [rows, cols])

    def to(self, device):
        self.cores = [c.to(device) for c in self.cores]
        return self

    def numpy(self):
        return self.torch().detach().cpu().numpy()

    def trace(self) -> torch.Tensor:
        """Trace of the matrix (matrix.py:160-175): the diagonal slices of every core summed, then a chain of small
        products; a scalar (batch: one per item)."""
        c5 = self.cores if self.batch else [c[None] for c in self.cores]
        ops = ops_for(c5[0])
        acc = None
        for c in c5:
            D = ops.diag_sum(c)  # [B, r0, r1]
            if acc is None:
                acc = D
            elif D.is_cuda:
                from . import _hip

                acc = _hip.gemm(acc, D)
            else:
                acc = torch.bmm(acc, D)
        if acc.shape[1] > 1:
            # a leading boundary rank > 1 is summed away: the reference starts from factor = ones(1), which einsum broadcasts
            # over the first rank index (matrix.py:160-175)
            if acc.is_cuda:
                from . import _hip

                acc = _hip.gemm(torch.ones((acc.shape[0], 1, acc.shape[1]), dtype=acc.dtype, device=acc.device), acc)
            else:
                acc = acc.sum(dim=1, keepdim=True)
        out = acc[:, 0, 0]
        return out if self.batch else out[0]


class CPMatrix:
    """Same constructor contract as ``tntorch.CPMatrix`` (matrix.py:340-387): ``M`` [rows, cols] is reshaped and interleaved as
    for ``TTMatrix`` and decomposed by ``Tensor(..., ranks_cp=rank)`` (CP-ALS; on device tensors the CP-ALS kernels); factor k
    ``[i_k o_k, R]`` is viewed as ``[i_k, o_k, R]``.  Beyond the reference: a list of such cores in place of ``M`` (``rank`` is
    then read from them and may be None), as ``TTMatrix`` takes pre-processed cores."""

    def __init__(self, M: Union[torch.Tensor, Sequence[torch.Tensor]], rank: Optional[int], input_dims: Sequence[int],
                 output_dims: Sequence[int], batch_size: int = 1, verbose: bool = False):
        assert len(input_dims) == len(output_dims)
        assert len(input_dims) > 0
        idims, odims = [int(x) for x in input_dims], [int(x) for x in output_dims]
        self.input_dims = torch.tensor(idims)
        self.output_dims = torch.tensor(odims)
        self.batch_size = batch_size
        self.d = len(idims)

        if isinstance(M, (list, tuple)):  # pre-processed cores [i_k, o_k, R]
            cores = list(M)
            assert len(cores) == self.d and all(c.dim() == 3 for c in cores)
            assert all(tuple(c.shape[:2]) == (idims[k], odims[k]) and c.shape[2] == cores[0].shape[2] for k, c in enumerate(cores))
            assert rank is None or int(rank) == cores[0].shape[2]
            self.rank = int(cores[0].shape[2])
            self.cores = cores
            return

        assert isinstance(rank, int)
        assert len(M.shape) == 2
        self.rank = rank
        rows, cols = 1, 1
        for a, b in zip(idims, odims):
            rows, cols = rows * a, cols * b
        assert rows == M.shape[0]
        assert cols == M.shape[1]
        tensor = M.reshape(idims + odims)
        perm = [k + off for k in range(self.d) for off in (0, self.d)]   # i_0 o_0 i_1 o_1 ... (matrix.py:373-381); a layout copy
        tensor = tensor.permute(perm).reshape([idims[k] * odims[k] for k in range(self.d)])
        if not tensor.is_contiguous():
            tensor = tensor.contiguous()
        cp = Tensor(tensor, ranks_cp=rank, verbose=verbose)
        self.cores = [c.reshape(idims[k], odims[k], c.shape[-1]) for k, c in enumerate(cp.cores)]

    def torch(self) -> torch.Tensor:
        """Decompress into a dense ``rows x cols`` matrix (matrix.py:389-410)."""
        idims, odims = self.input_dims.tolist(), self.output_dims.tolist()
        dense = Tensor([c.reshape(-1, c.shape[-1]) for c in self.cores]).torch()
        dense = dense.reshape([x for k in range(self.d) for x in (idims[k], odims[k])])
        perm = [2 * k for k in range(self.d)] + [2 * k + 1 for k in range(self.d)]
        rows, cols = int(torch.prod(self.input_dims)), int(torch.prod(self.output_dims))
        return dense.permute(perm).reshape(rows, cols)

    def to(self, device):
        self.cores = [c.to(device) for c in self.cores]
        return self

    def numpy(self):
        return self.torch().detach().cpu().numpy()


def _multiply_operands(who: str, kind, matrix, tensor: torch.Tensor, core_dims: int):
    """The checks ``tt_multiply`` and ``cp_multiply`` share; returns (x2d [b, rows], cols)."""
    if not isinstance(matrix, kind):
        raise ValueError("{}: the first argument must be a {}, got {}".format(who, kind.__name__, type(matrix).__name__))
    if not isinstance(tensor, torch.Tensor) or tensor.dim() < 2:
        raise ValueError("{}: the tensor needs at least 2 dimensions (reshape a vector to [1, rows])".format(who))
    cores = matrix.cores
    if any(c.dim() != core_dims for c in cores):
        raise ValueError("{}: batched matrices ({}-D cores) are not supported".format(who, cores[0].dim()))
    if tensor.dtype not in (torch.float32, torch.float64):
        raise ValueError("{}: float32 or float64 operands are needed, got {}".format(who, tensor.dtype))
    if any(c.dtype != tensor.dtype for c in cores):
        raise ValueError("{}: the matrix and the tensor must have the same dtype".format(who))
    if any(c.device != tensor.device for c in cores):
        raise ValueError("{}: the matrix and the tensor must be on the same device".format(who))
    io = 1 if core_dims == 4 else 0   # where the input mode sits in a core
    rows, cols = 1, 1
    for c in cores:
        rows, cols = rows * int(c.shape[io]), cols * int(c.shape[io + 1])
    if tensor.numel() % rows != 0:
        raise ValueError("{}: the tensor has {} elements, not a multiple of the matrix's {} rows".format(who, tensor.numel(), rows))
    return tensor.reshape(-1, rows), cols


def tt_multiply(tt_matrix: TTMatrix, tensor: torch.Tensor) -> torch.Tensor:
    """``tensor.reshape(b, rows) @ tt_matrix.torch()`` -> ``[b, cols]`` on the operands' device in their dtype, without forming
    the matrix (matrix.py:420-443): ``d`` steps, on the device one ``ttr_ttm_step`` launch each.  ``tensor`` has at least 2
    dimensions and a multiple of ``rows`` elements (a vector is ``[1, rows]``); neither operand is modified.  With grad mode on
    and a device core or tensor that requires grad the result carries a backward pass (``autodiff.tt_matvec``): the same forward
    launches and bits, then one ``ttr_ttm_grad_core`` per core and one ``ttr_ttm_grad_input`` per step that need a gradient."""
    x2d, cols = _multiply_operands("tt_multiply", TTMatrix, tt_matrix, tensor, 4)
    cores = tt_matrix.cores
    if cores[0].shape[0] != 1 or cores[-1].shape[-1] != 1:
        raise ValueError("tt_multiply: the boundary ranks must be 1, got {} and {}".format(cores[0].shape[0], cores[-1].shape[-1]))
    if x2d.shape[0] == 0:
        return torch.zeros((0, cols), dtype=tensor.dtype, device=tensor.device)
    if x2d.device.type != "cpu" and torch.is_grad_enabled() and (x2d.requires_grad or any(c.requires_grad for c in cores)):
        from . import autodiff

        return autodiff.tt_matvec(cores, x2d, ops_for(x2d, grad=True))
    return ops_for(x2d).tt_matvec_chain(cores, x2d)


def cp_multiply(cp_matrix: CPMatrix, tensor: torch.Tensor) -> torch.Tensor:
    """``tensor.reshape(b, rows) @ cp_matrix.torch()`` -> ``[b, cols]`` (matrix.py:446-468): ``d`` steps that carry the rank
    index, on the device one ``ttr_cpm_step`` launch each, and the sum over the rank (``ttr_mode_reduce``).  Not differentiable
    on the device: under grad mode an operand there that requires grad raises ``NotImplementedError``."""
    x2d, cols = _multiply_operands("cp_multiply", CPMatrix, cp_matrix, tensor, 3)
    if x2d.shape[0] == 0:
        return torch.zeros((0, cols), dtype=tensor.dtype, device=tensor.device)
    if x2d.device.type != "cpu" and torch.is_grad_enabled() and any(c.requires_grad for c in cp_matrix.cores):
        # (a tensor that requires grad is refused by ops_for; cores that do would come back detached, silently)
        raise NotImplementedError("tntorch_amd: cp_multiply is not differentiable on the device; detach the cores or use CPU tensors")
    return ops_for(x2d).cp_matvec_chain(cp_matrix.cores, x2d)

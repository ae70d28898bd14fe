"""Maximum-volume row selection (maxvol.py:115-170, ``py_maxvol``): the pivot rule of TT-cross.

``maxvol(A)`` returns the ``r`` rows ``index`` of a tall ``[N, r]`` matrix (or each matrix of a ``[B, N, r]`` batch) whose
submatrix has locally maximal volume, and ``C = A A[index]^-1``.  The start is LU with partial pivoting (getrf's pivots); then
Sherman-Morrison-Woodbury row swaps run while ``max |C| > tol`` and fewer than ``max_iters`` swaps were made.  The pivot of a
swap is the first maximum of ``|C^T|`` in row-major order, as in the reference (``divmod(abs(C).argmax(), N)``).

CPU tensors run the host mirror (``_hostops.maxvol``: ``torch.linalg.lu_factor`` = LAPACK getrf, the rank-1 updates in torch;
C is the updated matrix, as in the reference).  Device tensors run ``ttr_maxvol`` (``csrc/ttr_maxvol.hip``), which solves the
final C fresh from the final rows and reads nothing back to the host.
"""

from __future__ import annotations

from typing import Tuple

import torch

from ._dispatch import ops_for

__all__ = ["maxvol"]


def maxvol(A: torch.Tensor, tol: float = 1.05, max_iters: int = 100) -> Tuple[torch.Tensor, torch.Tensor]:
    """``A`` [N, r] or [B, N, r] -> ``(index, C)``: ``index`` int64 [r] / [B, r], ``C`` [N, r] / [B, N, r].
    ``N <= r`` returns ``arange(N)`` and the identity (maxvol.py:128-129)."""
    if not isinstance(A, torch.Tensor):
        A = torch.as_tensor(A)
    if A.dim() not in (2, 3):
        raise ValueError("maxvol: A must be [N, r] or [B, N, r]")
    batched = A.dim() == 3
    A3 = A if batched else A[None]
    B, N, r = A3.shape
    if tol < 1:
        tol = 1.0
    if N <= r:
        index = torch.arange(N, device=A.device).expand(B, N).clone()
        C = torch.eye(N, dtype=A.dtype, device=A.device).expand(B, N, N).clone()
    else:
        index, C = ops_for(A3).maxvol(A3, float(tol), int(max_iters))
    return (index, C) if batched else (index[0], C[0])

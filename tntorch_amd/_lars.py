"""Least angle regression on the normal equations: the coefficient path of LARS from ``G = M^T M`` and ``b = M^T y`` alone.

``PCEInterpolator.fit`` (interpolation.py:505-530 of the reference) calls ``sklearn.linear_model.Lars(fit_intercept=False)``
on the P x C design matrix.  Everything LARS needs from the data is in the C x C Gram matrix and the C correlations, so the
fit here never sees ``M`` or ``y``: the device forms ``(G, b)``, and this module walks the path on the host in fp64.

Plain LARS (Efron et al., "Least angle regression", 2004), no lasso drops, with scikit-learn's conventions so that the path is
the one ``Lars(...).coef_path_`` gives: the sign of a variable is that of its correlation when it enters; the step is the
smallest positive one to the next equi-correlated candidate (``min+`` of ``(C - c_j) / (A - a_j)`` and ``(C + c_j) / (A + a_j)``,
capped by ``C / A``), the correlations with the equiangular direction rounded to 15 decimals as scikit-learn does; the Cholesky
factor of the active Gram matrix grows by one row per step; when an active coefficient would cross zero within the step, its
sign flips and the next step adds no variable.  Two rules differ on purpose: a candidate whose Cholesky pivot falls below 1e-7
is excluded from all later steps (scikit-learn zeroes its correlation once), and the path stops when ``max|c| / n_samples``
falls to 2.2e-16 (scikit-learn stops at the fp32 epsilon, which ends an exactly representable fit seven digits early).
"""

from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

__all__ = ["lars_path"]

_TINY32 = float(np.finfo(np.float32).tiny)   # keeps the step's denominators off zero, as in scikit-learn
_EPS = float(np.finfo(np.float64).eps)
_PIVOT_MIN = 1e-7
_DECIMALS = int(np.finfo(np.float64).precision)


def _min_pos(x: np.ndarray) -> float:
    x = x[x > 0]
    return float(x.min()) if x.size else float(np.finfo(np.float64).max)


def _solve_lower(L: np.ndarray, rhs: np.ndarray, trans: bool = False) -> np.ndarray:
    Lt = torch.from_numpy(L.T if trans else L)
    return torch.linalg.solve_triangular(Lt, torch.from_numpy(np.ascontiguousarray(rhs))[:, None], upper=trans)[:, 0].numpy()


def lars_path(G, b, n_samples: int = 1, max_steps: Optional[int] = None) -> Tuple[np.ndarray, List[int]]:
    """The LARS path of ``min ||M x - y||`` from ``G = M^T M`` ([C, C]) and ``b = M^T y`` ([C]).

    :param G: the Gram matrix (array or tensor of any float dtype; converted to fp64, not modified)
    :param b: the correlations of the columns with the target
    :param n_samples: number of rows of ``M``: the path stops when ``max|c| / n_samples <= 2.2e-16``
    :param max_steps: stop after this many steps (None: until every candidate is active)
    :return: (path [C, steps + 1] in fp64, column 0 all zeros; the candidates in the order they became active)
    """
    G = np.array(torch.as_tensor(G).detach().cpu().double().numpy(), dtype=np.float64)
    cov = np.array(torch.as_tensor(b).detach().cpu().double().numpy(), dtype=np.float64).reshape(-1)
    C = cov.shape[0]
    if G.shape != (C, C):
        raise ValueError("lars_path: G must be [C, C] and b [C], got {} and {}".format(G.shape, cov.shape))
    max_steps = C if max_steps is None else max(0, min(int(max_steps), C))
    L = np.zeros((max_steps, max_steps))
    active: List[int] = []
    signs: List[float] = []
    free = np.ones(C, dtype=bool)       # neither active nor excluded
    coefs = [np.zeros(C)]
    drop = False
    steps = 0
    while True:
        cand = np.nonzero(free)[0]
        if cand.size:
            j = int(cand[np.argmax(np.abs(cov[cand]))])
            c_j, Cmax = cov[j], abs(cov[j])
        else:
            j, c_j, Cmax = -1, 0.0, 0.0
        if Cmax / n_samples <= _EPS:
            break
        if steps >= max_steps or len(active) >= C:
            break
        if not drop:
            # append row j to the Cholesky factor of the active Gram matrix
            n = len(active)
            row = _solve_lower(L[:n, :n], G[j, active]) if n else np.zeros(0)
            diag = max(np.sqrt(abs(G[j, j] - float(np.dot(row, row)))), _EPS)
            if diag < _PIVOT_MIN:    # degenerate with the active set: never considered again
                free[j] = False
                continue
            L[n, :n] = row
            L[n, n] = diag
            active.append(j)
            signs.append(float(np.sign(c_j)))
            free[j] = False
        n = len(active)
        sg = np.array(signs)
        ls = _solve_lower(L[:n, :n], _solve_lower(L[:n, :n], sg), trans=True)
        if n == 1 and ls[0] == 0:
            ls[0] = 1.0
            AA = 1.0
        else:
            AA = 1.0 / np.sqrt(float(np.sum(ls * sg)))
            ls = ls * AA
        rest = np.nonzero(free)[0]
        corr = np.around(G[np.ix_(active, rest)].T @ ls, decimals=_DECIMALS)
        g1 = _min_pos((Cmax - cov[rest]) / (AA - corr + _TINY32))
        g2 = _min_pos((Cmax + cov[rest]) / (AA + corr + _TINY32))
        gamma = min(g1, g2, Cmax / AA)
        prev = coefs[-1]
        z = -prev[active] / (ls + _TINY32)
        z_pos = _min_pos(z)
        drop = False
        if z_pos < gamma:    # an active coefficient changes sign within the step: its sign flips, the next step adds nothing
            for i in np.nonzero(z == z_pos)[0]:
                signs[int(i)] = -signs[int(i)]
            drop = True
        new = np.zeros(C)
        new[active] = prev[active] + gamma * ls
        coefs.append(new)
        steps += 1
        cov[rest] -= gamma * corr    # the correlations of the candidates with the new residual
    return np.stack(coefs, axis=1), active

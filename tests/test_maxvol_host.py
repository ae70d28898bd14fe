"""A plain fp64 maxvol written from the documented rules (include/ttround_hip.h, ttr_maxvol), with a record of every pivot
decision, and its checks on the CPU: it reproduces tests/golden/maxvol_f64.npz, and it and the host mirror reproduce the
reference's rows on the exactly tied inputs of tests/golden/maxvol_ties_f64.npz (tools/gen_maxvol_ties.py).  The GPU tests
(test_maxvol_gpu.py) compare ttr_maxvol with it."""
import os
from dataclasses import dataclass, field

import numpy as np
import pytest
import torch

import tntorch_amd as tn
from tools.gen_cross_golden import MAXVOL_CASES, maxvol_input
from tools.gen_maxvol_ties import tie_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@dataclass
class Decision:
    kind: str      # "lu" (pivot of one column), "swap" (pivot of one swap) or "stop" (|C| max against tol)
    step: int
    tied: bool     # the winner has a bitwise-equal competitor
    gap: float     # relative distance of the winner to the best candidate not tied with it (inf: none)


@dataclass
class MaxvolResult:
    index: np.ndarray
    C: np.ndarray
    swaps: int
    decisions: list = field(default_factory=list)

    def decision(self, kind, step):
        return next(d for d in self.decisions if d.kind == kind and d.step == step)

    def min_gap(self):
        """Smallest relative gap over all decisions (ties are measured against the best non-tied candidate)."""
        return min(d.gap for d in self.decisions)


def _decide(vals, kind, step):
    """First maximum of `vals` (already in the order of the tie rule) and its Decision."""
    j = int(np.argmax(vals))
    v = vals[j]
    others = vals[vals != v]
    gap = np.inf if others.size == 0 or v == 0 else (v - others.max()) / v
    return j, Decision(kind, step, int((vals == v).sum()) > 1, float(gap))


def ref_maxvol(A, tol=1.05, max_iters=100):
    """maxvol of A [N, r] in fp64 by the documented rules:
    - start: unblocked right-looking LU with explicit row swaps (dgetf2); the pivot of column k is the first maximum of |W[k:, k]|
      in the current (permuted) order, so ties go to the first position;
    - swaps (Sherman-Morrison-Woodbury) while max |C| > tol and fewer than max_iters swaps: the pivot is the first maximum of
      |C^T| in row-major order (key q * N + n);
    - every decision is recorded with its gap (Decision)."""
    A = np.asarray(A, dtype=np.float64)
    N, r = A.shape
    tol = max(tol, 1.0)
    if N <= r:
        return MaxvolResult(np.arange(N), np.eye(N), 0)
    W = A.copy()
    perm = np.arange(N)  # perm[position] = row
    decisions = []
    for k in range(r):
        j, d = _decide(np.abs(W[k:, k]), "lu", k)
        decisions.append(d)
        j += k
        W[[k, j]] = W[[j, k]]
        perm[[k, j]] = perm[[j, k]]
        if W[k, k] != 0:
            W[k + 1:, k] /= W[k, k]
            W[k + 1:, k + 1:] -= np.outer(W[k + 1:, k], W[k, k + 1:])
    index = perm[:r].copy()
    C = np.linalg.solve(A[index].T, A.T).T
    swaps = 0
    while True:
        flat, d = _decide(np.abs(C.T).reshape(-1), "swap", swaps)
        q, p = divmod(flat, N)
        v = abs(C[p, q])
        stop = Decision("stop", swaps, False, abs(v - tol) / tol)
        if not v > tol or swaps >= max_iters:
            decisions.append(stop)
            break
        decisions += [d, stop]
        index[q] = p
        x = C[p].copy()
        x[q] -= 1.0
        C += np.outer(C[:, q] * (-1.0 / C[p, q]), x)
        swaps += 1
    return MaxvolResult(index, C, swaps, decisions)


def assert_gaps(res, thr, name=""):
    """Every decision of `res` is decided by a margin of at least `thr` (exact ties count by their best non-tied competitor)."""
    bad = [d for d in res.decisions if not d.gap >= thr]
    assert not bad, f"{name}: decisions closer than {thr}: {bad[:3]}"


def load_ties():
    g = np.load(os.path.join(GOLDEN, "maxvol_ties_f64.npz"))
    return {name: (A, it, tied, g[f"{name}_index"]) for name, (A, it, tied) in tie_cases().items()}


def test_ref_matches_golden():
    g = np.load(os.path.join(GOLDEN, "maxvol_f64.npz"))
    for k, (N, r, it) in enumerate(MAXVOL_CASES):
        res = ref_maxvol(maxvol_input(k, N, r), max_iters=it)
        np.testing.assert_array_equal(res.index, g[f"m{k}_index"], err_msg=f"case {k}: {(N, r, it)}")
        if N > r:
            assert_gaps(res, 1e-6, f"case {k}")
            assert res.swaps == min(it, res.swaps)


def test_ties_are_ties():
    """The named decision of every tie case is an exact tie in the reference's rows, and all the others hold their gap."""
    for name, (A, it, tied, index) in load_ties().items():
        res = ref_maxvol(A, max_iters=it)
        assert res.decision(*tied).tied, name
        assert_gaps(res, 1e-6, name)
        np.testing.assert_array_equal(res.index, index, err_msg=name)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_ties_host_mirror(dtype):
    for name, (A, it, tied, index) in load_ties().items():
        i, C = tn.maxvol(torch.as_tensor(A).to(dtype), max_iters=it)
        np.testing.assert_array_equal(i.numpy(), index, err_msg=name)


def test_tie_rules_by_construction():
    """The cases pin the rules they are named after: the first ROW (instead of position) or the row-major key of C (instead of
    C^T) would choose differently."""
    ties = load_ties()
    A, it, _, index = ties["lu_block"]  # rows 0 and 3 equal; pivot 0 (row 5) moved row 0 to position 5
    assert index[0] == 5 and index[1] == 3
    A, it, _, index = ties["swap_cross_col"]  # C[29, 0] = 9/8 = C[7, 1]: column 0 comes first
    res = ref_maxvol(A, max_iters=it)
    C0 = np.linalg.solve(A[:3].T, A.T).T
    assert C0[29, 0] == C0[7, 1] == 9 / 8
    assert index[0] == 29 and res.swaps >= 1


def test_ref_edges():
    """Degenerate inputs of the reference itself: N <= r, tol clamp, max_iters = 0."""
    res = ref_maxvol(np.ones((3, 4)))
    assert list(res.index) == [0, 1, 2] and res.swaps == 0
    A = maxvol_input(3, 64, 8)
    assert ref_maxvol(A, tol=0.5).swaps == ref_maxvol(A, tol=1.0).swaps
    assert ref_maxvol(A, max_iters=0).swaps == 0

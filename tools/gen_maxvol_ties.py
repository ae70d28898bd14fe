"""Record tests/golden/maxvol_ties_f64.npz from the unmodified reference (tntorch's py_maxvol; CPU, fp64): maxvol inputs whose
pivots are decided by exact ties, so that the tie rules are pinned down.

    python tools/gen_maxvol_ties.py /path/to/tntorch-checkout

The inputs are built by tie_cases() (the tests rebuild them; only the chosen rows are stored).  Every value that meets a tie is
exact under any rounding: duplicated and negated rows (each row of the elimination and of C goes through the same operations),
or dyadic values with a few bits (A = L D with D a power-of-two diagonal, so that the LU, A[index]^-1 and C are exact in fp32 and
fp64).  The cases:
- lu_*: getrf's pivot of column 1 is tied between a row and its copy; pivot 0 moved the smaller row to a LATER position, so the
  first position (getrf) and the first row disagree.  In one 16-row block, across blocks, and across the 256 argmax partials of
  the kernel (N > 4096).
- swap_same_col: the first swap is tied between a row and its copy (and its negation) in the same column of C.
- swap_cross_col: the first swap is tied between C[n1, 0] and C[n2, 1] with n1 > n2: the key q * N + n (column first) picks n1.
The generator checks with the test reference (tests/test_maxvol_host.py) that the named decision of each case is a tie (the
winner has a bitwise-equal competitor) and that the reference's rows are the recorded ones.  Only data is written.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "maxvol_ties_f64.npz")


def _lu_dup(N, r, b, p0, seed, negate=False):
    """Small random A; row p0 is pivot 0 (so getrf's swap moves row 0 to position p0); row b (0 < b < p0) is a copy of row 0
    (negated with `negate`) with the largest column-1 entry: getrf's pivot 1 is row b (position b < p0), the first ROW is 0."""
    a = 0
    rng = np.random.default_rng(seed)
    A = 0.1 * rng.standard_normal((N, r))
    A[p0, 0] = 4.0
    A[a] = 0.1 * rng.standard_normal(r)
    A[a, 1] = 2.0
    A[b] = -A[a] if negate else A[a]
    return A


def _dyadic(N, planted, seed):
    """A = L D, r = 3: rows 0 .. 2 are L11 = [[1, 0, 0], [1/2, 1, 0], [1/2, 1/2, 1]], the other rows of L are multiples of 1/8
    in [-1/4, 1/4], D = diag(2, 4, 1/2).  The LU start picks rows 0, 1, 2 with pivots 2, 4, 1/2 and no tie, and C = L L11^-1,
    all exact.  `planted` {row: L row} sets chosen rows; the random rows have |C| <= 7/16."""
    rng = np.random.default_rng(seed)
    L = rng.integers(-2, 3, (N, 3)) / 8.0
    L[:3] = [[1, 0, 0], [0.5, 1, 0], [0.5, 0.5, 1]]
    for row, v in planted.items():
        L[row] = v
    return L * np.array([2.0, 4.0, 0.5])


def tie_cases():
    """name -> (A [N, r] fp64, max_iters, the tied decision: ("lu", column) or ("swap", swap number))."""
    c0 = [0.75, -0.5, -0.5]  # C row (9/8, -1/4, -1/2)
    c1 = [0.0, 0.75, -0.75]  # C row (-3/16, 9/8, -3/4)
    return {
        "lu_block": (_lu_dup(8, 3, 3, 5, 1), 100, ("lu", 1)),
        "lu_block_neg": (_lu_dup(8, 3, 3, 5, 2, negate=True), 100, ("lu", 1)),
        "lu_blocks": (_lu_dup(48, 5, 20, 40, 3), 100, ("lu", 1)),
        "lu_partials": (_lu_dup(4500, 4, 4100, 4400, 4, negate=True), 100, ("lu", 1)),
        "swap_same_col": (_dyadic(40, {9: c0, 25: c0}, 5), 100, ("swap", 0)),
        "swap_same_col_neg": (_dyadic(40, {9: c0, 25: [-x for x in c0]}, 6), 100, ("swap", 0)),
        "swap_cross_col": (_dyadic(40, {29: c0, 7: c1}, 7), 100, ("swap", 0)),
        "swap_cross_col_blocks": (_dyadic(5000, {4500: c0, 30: c1}, 8), 100, ("swap", 0)),
    }


def main(ref):
    sys.path.insert(0, ref)
    sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT]
    from tntorch.maxvol import py_maxvol
    from test_maxvol_host import ref_maxvol

    out = {}
    for name, (A, it, tied) in tie_cases().items():
        index, C = py_maxvol(A, max_iters=it)
        res = ref_maxvol(A, max_iters=it)
        d = res.decision(*tied)
        assert d.tied, f"{name}: decision {tied} is not a tie"
        assert np.array_equal(index.astype(np.int64), res.index), f"{name}: test reference {res.index} != reference {index}"
        out[f"{name}_index"] = index.astype(np.int64)
        print(f"{name}: index {index.tolist()}, swaps {res.swaps}")
    np.savez_compressed(OUT, **out)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

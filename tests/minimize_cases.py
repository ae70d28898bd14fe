"""The cases of tests/golden/minimize_f64.npz (tools/gen_minimize_golden.py), shared by the host and the GPU tests of
``tn.minimum`` / ``tn.argmin`` / ``tn.maximum`` / ``tn.argmax``.  A case is a dense fp64 tensor built with torch and the train
made from it (``tn.Tensor(dense)``: the identity-padded full-rank train, which holds every entry exactly; ``sinquad`` at
``ranks_tt=8``; ``randn3`` is a random train and its own dense tensor).  ``tn`` is the package that builds the train: this one in
the tests, the reference in the recording tool."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 1, 2)
FUNCTIONS = ("minimum", "argmin", "maximum", "argmax")
CASES = ("quad8", "quad5764", "sinquad", "randn3")
UNIQUE = ("quad8", "quad5764", "randn3")   # one optimiser each; sinquad has several exactly tied ones
EXACT_TRAIN = ("quad8", "quad5764")        # trains whose entries ARE the dense entries (products with 0 and 1 only)

# |minimum - the reference's minimum| / |minimum| over CASES x SEEDS x (minimum, maximum) stays below this: 4 x the largest
# deviation found against minimize_f64.npz.  Measured on the CPU: 1.80e-15 (quad8, seed 0, minimum: the reference returned
# 0.6799999999999988 for 0.68, its tan(pi/2 - y) + min round trip; 13 of the 24 pairs agree exactly, sinquad all six).
REF_MEASURED = 1.80e-15
REF_RTOL = 4 * REF_MEASURED

# fp32 on the device: |minimum - dense.min()| and dense[argmin] - dense.min() relative to max |dense| stay below this: 4 x the
# largest deviation measured over CASES x SEEDS x the four functions on an MI355X (tests/test_cross_gpu.py has no fp32
# device-against-dense comparison of values to take it from).  Measured: 2.23e-7 (randn3; fp32 eps is 1.19e-7).
FP32_MEASURED = 2.23e-7
FP32_RTOL = 4 * FP32_MEASURED

_Z = None


def fixture():
    global _Z
    if _Z is None:
        with np.load(os.path.join(ROOT, "tests", "golden", "minimize_f64.npz")) as z:
            _Z = {k: z[k] for k in z.files}
    return _Z


def _quad(shape, c, offset):
    grids = torch.meshgrid(*[torch.arange(s, dtype=torch.float64) for s in shape], indexing="ij")
    return sum((x - ci) ** 2 for x, ci in zip(grids, c)) + offset


def dense(name):
    """The dense fp64 tensor of a case (None for randn3: its train comes first)."""
    if name == "quad8":
        return _quad([8] * 4, (2.2, 5.1, 0.3, 6.8), 0.5)
    if name == "quad5764":
        return _quad([5, 7, 6, 4], (3.6, 1.2, 4.9, 0.1), 0.5)
    if name == "sinquad":
        q = _quad([6] * 5, (1.1, 4.2, 2.7, 0.4, 3.3), 0.5)
        return 3 * torch.sin(q) + 0.2 * q
    if name == "quad8_zero":   # minimum exactly 0, at (2, 5, 0, 7)
        return _quad([8] * 4, (2, 5, 0, 7), 0.0)
    assert name == "randn3"
    return None


def build(name, tn):
    """(train, dense) of a case in fp64 on the CPU, the train built by the package ``tn`` (default dtype fp64 for the call)."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        if name == "randn3":
            torch.manual_seed(7)
            t = tn.randn([6] * 4, ranks_tt=3)
            return t, t.torch()
        d = dense(name)
        return (tn.Tensor(d, ranks_tt=8) if name == "sinquad" else tn.Tensor(d)), d
    finally:
        torch.set_default_dtype(old)


def value_bound(t, pos):
    """How far two evaluations of the train ``t`` at ``pos`` can lie apart in t's dtype, whatever the order of their products
    (a fibre sample is left interface x core x right interface, ``t[pos]`` a chain from the left): each is within
    gamma_n S of the exact entry, S the entry of the train of absolute values, n the sum of the ranks (the terms of all inner
    products), so they differ by at most 2 n eps S (to first order; the 2 is kept as the margin for the second)."""
    S = torch.ones(1, 1, dtype=torch.float64)
    for c, p in zip(t.cores, pos):
        S = S @ c[:, int(p), :].double().abs().cpu()
    n = sum(int(c.shape[0]) for c in t.cores)
    return 2 * n * torch.finfo(t.cores[0].dtype).eps * float(S)


def seed(s):
    torch.manual_seed(s)
    np.random.seed(s)


def to(t, tn, dtype, device):
    return tn.Tensor([c.to(dtype).to(device) for c in t.cores])

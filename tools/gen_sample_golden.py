"""Record tests/golden/sample_f64.npz from the unmodified reference (tntorch; CPU, fp64 default dtype, fixed seeds), as
tools/gen_minimize_golden.py does for the minimisation.

    python tools/gen_sample_golden.py /path/to/tntorch-checkout

For every case of tests/sample_cases.py (CASES): the cores of the train as the reference drew them after
``torch.manual_seed(11)`` (``<case>_core<n>``) and the reference's ``tn.sample(t, P=4096, seed=5)`` as uint8 (``<case>_X``; every
mode size is at most 64).  Also printed, not stored: in how many rows the reference's own fp32 run (cores cast) differs from its
fp64 run.  Only data is written; no reference code is copied.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "sample_f64.npz")


def main(ref):
    sys.path.insert(0, ref)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tntorch as tn

    import sample_cases as sc

    out = {}
    for name in sc.CASES:
        torch.set_default_dtype(torch.float64)
        t = sc.build(name, tn)
        for n, c in enumerate(t.cores):
            out[f"{name}_core{n}"] = c.numpy()
        X = tn.sample(t, P=sc.P_GOLDEN, seed=sc.SEED_GOLDEN).numpy()
        assert X.min() >= 0 and X.max() < 256 and (X == np.round(X)).all()
        out[f"{name}_X"] = X.astype(np.uint8)
        torch.set_default_dtype(torch.float32)
        X32 = tn.sample(tn.Tensor([c.float() for c in t.cores]), P=sc.P_GOLDEN, seed=sc.SEED_GOLDEN).numpy()
        print(f"{name}: the reference's fp32 run differs from its fp64 run in {int((X32 != X).any(axis=1).sum())} of {sc.P_GOLDEN} rows")
    torch.set_default_dtype(torch.float64)
    np.savez_compressed(OUT, **out)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

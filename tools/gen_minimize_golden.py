"""Record tests/golden/minimize_f64.npz from the unmodified reference (tntorch; CPU, fp64 default dtype, fixed seeds), as
tools/gen_cross_golden.py does for cross.

    python tools/gen_minimize_golden.py /path/to/tntorch-checkout

For every case of tests/minimize_cases.py (CASES), seed (SEEDS) and function (minimum, argmin, maximum, argmax), called with the
reference's default arguments after ``torch.manual_seed(s); np.random.seed(s)``: the value or the position it returned
(``<case>_s<seed>_<function>``) and, from one ``cross(..., _minimize=True, return_info=True)`` call with the same seed and the
defaults of ``minimum``, the number of samples (``<case>_s<seed>_nsamples``).  Also the dense tensor's optimum and the cores of the
random train ``randn3`` (``randn3_core<n>``), so that the tests can tell whether this package draws the same train.  The reference's
``cross`` uses ``np.int``, which NumPy no longer has: ``np.int = int`` is set here, the reference itself is not touched.  Only data
is written; no reference code is copied.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "minimize_f64.npz")


def main(ref):
    sys.path.insert(0, ref)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    if not hasattr(np, "int"):
        np.int = int
    import tntorch as tn

    import minimize_cases as mc

    torch.set_default_dtype(torch.float64)
    out = {}
    for name in mc.CASES:
        t, d = mc.build(name, tn)
        if name == "randn3":
            for n, c in enumerate(t.cores):
                out[f"randn3_core{n}"] = c.numpy()
        out[f"{name}_dense_min"], out[f"{name}_dense_max"] = d.min().numpy(), d.max().numpy()
        worst = 0.0
        for s in mc.SEEDS:
            for fn in mc.FUNCTIONS:
                mc.seed(s)
                r = getattr(tn, fn)(t)
                out[f"{name}_s{s}_{fn}"] = np.asarray(r, dtype=np.int64) if fn.startswith("arg") else np.asarray(float(r))
                if fn.startswith("arg"):
                    hit = float(d[tuple(int(x) for x in r)])
                    assert hit == float(d.min() if fn == "argmin" else d.max()), (name, s, fn, r)
                else:
                    want = float(d.min() if fn == "minimum" else d.max())
                    worst = max(worst, abs(float(r) - want) / abs(want))
            mc.seed(s)
            _, info = tn.cross(tensors=t, function=lambda x: x, rmax=10, max_iter=10, verbose=False, return_info=True, _minimize=True)
            out[f"{name}_s{s}_nsamples"] = np.array(info["nsamples"])
        print(f"{name}: reference value against the dense optimum, worst relative deviation {worst:.2e}")
    np.savez_compressed(OUT, **out)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

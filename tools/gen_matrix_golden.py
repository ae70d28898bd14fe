"""Record tests/golden/matrix_f64.npz from the unmodified reference (tntorch; CPU, fp64 default dtype, fixed seeds), as
tools/gen_sample_golden.py does for the sampling.

    python tools/gen_matrix_golden.py /path/to/tntorch-checkout

For every case of tests/matrix_cases.py (CASES): the matrix and the input as ``matrix_cases.draw_matrix`` draws them
(``<case>_M``, ``<case>_x``), the cores of the reference's ``TTMatrix(M, ranks, ...)`` (``<case>_tt<k>``) and of its
``CPMatrix(M, cp_rank, ...)`` (``<case>_cp<k>``) as the reference built them, and its ``tt_multiply`` / ``cp_multiply`` outputs
(``<case>_tty``, ``<case>_cpy``).  Also printed, not stored: how far each recorded output is from ``x @ matrix.torch()``.
Only data is written; no reference code is copied.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "matrix_f64.npz")


def main(ref):
    sys.path.insert(0, ref)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tntorch as tn

    import matrix_cases as mc

    torch.set_default_dtype(torch.float64)
    out = {}
    for name, (idims, odims, ranks, cp_rank, _) in mc.CASES.items():
        M, x = mc.draw_matrix(name)
        out[name + "_M"], out[name + "_x"] = M.numpy(), x.numpy()
        torch.manual_seed(mc.SEED)
        ttm = tn.TTMatrix(M, list(ranks), idims, odims)
        for k, c in enumerate(ttm.cores):
            out[f"{name}_tt{k}"] = c.numpy()
        y = tn.tt_multiply(ttm, x)
        out[name + "_tty"] = y.numpy()
        print(f"{name}: tt ranks {[int(c.shape[-1]) for c in ttm.cores[:-1]]}, |tt_multiply - x @ torch()| = "
              f"{float((y - x @ ttm.torch()).abs().max()):.2e}")
        torch.manual_seed(mc.SEED)
        cpm = tn.CPMatrix(M, cp_rank, idims, odims)
        for k, c in enumerate(cpm.cores):
            out[f"{name}_cp{k}"] = c.numpy()
        y = tn.cp_multiply(cpm, x)
        out[name + "_cpy"] = y.numpy()
        print(f"{name}: cp rank {cp_rank}, |cp_multiply - x @ torch()| = {float((y - x @ cpm.torch()).abs().max()):.2e}")
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

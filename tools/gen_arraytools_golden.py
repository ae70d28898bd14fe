"""Record tests/golden/arraytools_f64.npz from the unmodified reference's array tools (``tools.py``: squeeze, unsqueeze, cat,
transpose, flip, unbind, ttm, generate_basis, pad; ``ops.cumsum``) on the CPU, with fixed seeds, as tools/gen_convolve_golden.py
does for the convolution.

    python tools/gen_arraytools_golden.py /path/to/tntorch-checkout

The default dtype is float64 while the reference runs, as in its own test_tools.py (its ``cat`` allocates default-dtype zeros).
All cores are drawn with ``rand`` in fp64 and stored (``<name>_ncores``, ``<name>_core<n>``, ``<name>_U<n>``).  Inputs:
  p   3x4x5, TT ranks 2            q   3x2x5, TT ranks 3          v   a one-mode tensor of size 4
  k   a 6x5 Tucker-TT: core modes 4x5, TT rank 2, one factor [6, 4] on mode 0
  b   3x4x2 with boundary ranks 2 (TT ranks 2, 3, 2, 2)           s   1x4x1x3, TT ranks 2
and the factors ``aux_<name>`` of ``AUX`` in tests/arraytools_cases.py.  Stored per case of ``CASES`` there:  out_<case>, the
reference's result densified in fp64 (a list of slices: stacked), and  basis_<name>_<I>x<K>  for ``generate_basis``.
The generator asserts that this package's CPU results match every case to 1e-13 (relative Frobenius).  Only data is written; no
reference code is copied.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SEED = 43


def rand_cores(shape, ranks, g, r0=1, rN=1):
    rs = [r0] + list(ranks) + [rN]
    return [torch.rand(rs[n], s, rs[n + 1], generator=g, dtype=torch.float64) for n, s in enumerate(shape)]


def main(ref):
    sys.path.insert(0, ref)
    import tntorch as ref_tn

    import arraytools_cases as ac
    import tntorch_amd as tn

    g = torch.Generator().manual_seed(SEED)
    inputs = {
        "p": (rand_cores([3, 4, 5], [2, 2], g), [None] * 3),
        "q": (rand_cores([3, 2, 5], [3, 3], g), [None] * 3),
        "k": (rand_cores([4, 5], [2], g), [torch.rand(6, 4, generator=g, dtype=torch.float64), None]),
        "b": (rand_cores([3, 4, 2], [3, 2], g, r0=2, rN=2), [None] * 3),
        "s": (rand_cores([1, 4, 1, 3], [2, 2, 2], g), [None] * 4),
        "v": (rand_cores([4], [], g), [None]),
    }
    assert tuple(inputs) == ac.TENSORS
    out = {}
    for name, (cores, Us) in inputs.items():
        out[name + "_ncores"] = np.array(len(cores))
        for n, c in enumerate(cores):
            out["{}_core{}".format(name, n)] = c.numpy()
            if Us[n] is not None:
                out["{}_U{}".format(name, n)] = Us[n].numpy()
    aux = {name: torch.randn(*shape, generator=g, dtype=torch.float64) for name, shape in ac.AUX.items()}
    for name, a in aux.items():
        out["aux_" + name] = a.numpy()

    def trains(module):
        return {name: module.Tensor([c.clone() for c in cores], Us=[None if U is None else U.clone() for U in Us])
                for name, (cores, Us) in inputs.items()}

    for case in ac.cases():
        torch.set_default_dtype(torch.float64)
        try:
            want = ac.dense(ac.CASES[case](ref_tn, trains(ref_tn), {k: a.clone() for k, a in aux.items()}))
        finally:
            torch.set_default_dtype(torch.float32)
        got = ac.dense(ac.CASES[case](tn, trains(tn), {k: a.clone() for k, a in aux.items()}))
        err = ac.rel_err(got, want)
        print("{:16s} shape {}  this package vs the reference {:.1e}".format(case, want.shape, err))
        assert err < 1e-13, "{}: this package is {:.2e} off the reference".format(case, err)
        out["out_" + case] = want
    for name in ac.BASES:
        for I, K in ac.BASIS_SHAPES:
            want = ref_tn.generate_basis(name, (I, K)).numpy()
            got = tn.generate_basis(name, (I, K)).numpy()
            assert want.dtype == np.float64 and got.dtype == np.float64
            err = float(np.abs(got - want).max())
            print("basis {:10s} {}x{}  this package vs the reference {:.1e}".format(name, I, K, err))
            assert err < 1e-13, (name, I, K, err)
            out["basis_{}_{}x{}".format(name, I, K)] = want
    np.savez_compressed(ac.GOLDEN, **out)
    print("wrote", ac.GOLDEN, os.path.getsize(ac.GOLDEN), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

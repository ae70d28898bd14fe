"""Record tests/golden/automata_f64.npz from the unmodified reference's ``automata``, ``logic``, ``tools.mask`` and
``derivatives.partialset`` (CPU, fixed seeds), as tools/gen_convolve_golden.py does for the convolution.

    python tools/gen_automata_golden.py /path/to/tntorch-checkout

Stored (trains as ``<name>_ncores``, ``<name>_core<n>`` in the dtype the reference builds, fp32):
  constructors   wm52 = weight_mask(5, 2); wm4 = weight_mask(4, [1, 3], nsymbols=3); wmv = weight_mask(3, [0, 2], nsymbols=[2, 3, 2]);
                 woh = weight_one_hot(4); wohr = weight_one_hot(3, r=2, nsymbols=3); w3 = weight(3); w23 = weight(2, nsymbols=3)
  dense_<f>      the dense values (fp64) of all / none / any / one / presence / absence on 4 symbols, without ``which`` and
                 with which = [1, 3] (suffix ``_w``; presence / absence only with it), and of only(x), only(x | z) on 4 symbols
  acc_<name>     accepted_inputs of wm52, wm4, w3, a zero tensor of 3 modes (``zero``, shape [0, 3]) and weight_mask(1, 1) (``n1``)
  (the two trains below have integer cores in {0, .., 3} and the steps are powers of two: every value is exact in fp64)
  mask_*         a 3x4x5 fp64 train of ranks 2 (``mask_t``) with idxs ``mask_idx<n>`` that exceed the mask's size in two modes, the
                 mask x | z on 3 symbols (``mask_m``) and the dense result (``mask_out``)
  pset_*         a 5x4x3 fp64 train of ranks 2 (``pset_t``), partialset(t, 1, mask=x, bounds=B) with B = ``pset_bounds``:
                 the dense result (``pset_out``) and its ``idxs`` (``pset_idx<n>``).  Order 1 only: for higher orders the
                 reference recomputes the step from the shrinking stack, which this package deliberately does not.
Only data is written; no reference code is copied.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "automata_f64.npz")
SEED = 43


def put_train(out, name, t):
    out[name + "_ncores"] = np.int64(len(t.cores))
    for n, c in enumerate(t.cores):
        out["{}_core{}".format(name, n)] = c.detach().numpy()


def rand_train(tn, shape, rank, g):
    rs = [1] + [rank] * (len(shape) - 1) + [1]
    return tn.Tensor([torch.randint(0, 4, (rs[n], s, rs[n + 1]), generator=g).double() for n, s in enumerate(shape)])


def main(ref_path):
    sys.path.insert(0, ref_path)
    import tntorch as tn

    out = {}
    g = torch.Generator().manual_seed(SEED)
    ctors = {
        "wm52": tn.automata.weight_mask(5, 2), "wm4": tn.automata.weight_mask(4, [1, 3], nsymbols=3),
        "wmv": tn.automata.weight_mask(3, [0, 2], nsymbols=[2, 3, 2]), "woh": tn.automata.weight_one_hot(4),
        "wohr": tn.automata.weight_one_hot(3, r=2, nsymbols=3), "w3": tn.automata.weight(3), "w23": tn.automata.weight(2, nsymbols=3),
    }
    for name, t in ctors.items():
        put_train(out, name, t)
    for f in ("all", "none", "any", "one"):
        out["dense_" + f] = getattr(tn, f)(4).torch().double().numpy()
        out["dense_" + f + "_w"] = getattr(tn, f)(4, [1, 3]).torch().double().numpy()
    for f in ("presence", "absence"):
        out["dense_" + f + "_w"] = getattr(tn, f)(4, [1, 3]).torch().double().numpy()
    x, y, z, w = tn.symbols(4)
    out["dense_only_x"] = tn.only(x).torch().double().numpy()
    out["dense_only_xz"] = tn.only(x | z).torch().double().numpy()
    for name in ("wm52", "wm4", "w3"):
        out["acc_" + name] = tn.automata.accepted_inputs(ctors[name]).numpy()
    out["acc_zero"] = tn.automata.accepted_inputs(tn.false(3)).numpy().reshape(0, 3)
    out["acc_n1"] = tn.automata.accepted_inputs(tn.automata.weight_mask(1, 1)).numpy()

    t = rand_train(tn, [3, 4, 5], 2, g)
    idxs = [np.array([0, 1, 2]), np.array([1, 0, 3, 1]), np.array([0, 0, 1, 4, 2])]
    t.idxs = idxs
    x3, y3, z3 = tn.symbols(3)
    m = x3 | z3
    put_train(out, "mask_t", t)
    put_train(out, "mask_m", m)
    for n in range(3):
        out["mask_idx{}".format(n)] = idxs[n]
    out["mask_out"] = tn.mask(t, m).torch().numpy()

    t = rand_train(tn, [5, 4, 3], 2, g)
    bounds = [[0.0, 2.0], [-3.0, 3.0], [0.0, 1.0]]   # steps 0.5, 2 and 0.5: every quotient is exact
    put_train(out, "pset_t", t)
    out["pset_bounds"] = np.array(bounds)
    p = tn.partialset(t, 1, mask=x3, bounds=bounds)
    out["pset_out"] = p.torch().numpy()
    for n in range(3):
        out["pset_idx{}".format(n)] = np.asarray(p.idxs[n]).astype(np.int64)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1])

"""Record tests/golden/convolve_f64.npz from the unmodified reference's ``tools.convolve`` (CPU, fp64 inputs, fixed seeds), as
tools/gen_derivatives_golden.py does for the differential operators.

    python tools/gen_convolve_golden.py /path/to/tntorch-checkout

All cores are drawn with ``rand`` in fp64 and stored (``<name>_ncores``, ``<name>_core<n>``, ``<name>_U<n>``).  Inputs:
  p   5x6x7, TT ranks 3            q   3x4x2, TT ranks 2          v, w   one-mode tensors of size 4
  m   5x1x4, TT ranks 2            n   1x6x4, TT ranks 2          g      a 3x3x3 rank-1 kernel
  k   a 6x5 Tucker-TT: core modes 4x5, TT rank 2, one factor [6, 4] on mode 0            h      3x2, TT rank 2
Pairs (``PAIRS``): p*q, q*p, v*w, m*n, k*h, p*g, each with mode 'full', 'same' and 'valid'.  Stored per case c = "<a><b>_<mode>":
  truth_c    scipy.signal.convolve(dense a, dense b, 'full') in fp64, cropped per mode to the window (lo, K) of the full result,
             k = min(I, J), m = max(I, J):  full (0, I + J - 1);  same ((k - 1) // 2, m);  valid (k - 1, m - k + 1)
             -- np.convolve's windows, which the reference's docstring names as its contract
  ref_c      the reference's result, densified, and  referr_c  its relative Frobenius error against truth_c, where the reference
             is well defined: it starts 'same' at k // 2 (numpy's window only for odd k) and its 'valid' slice [k-1 : -(k-1)]
             is empty for k = 1.  For the other cases only the truth is stored, and  truthonly_c = 1  marks the key.
The reference multiplies in the Fourier domain with three randomised TT-cross runs, so the seeds of torch and numpy are fixed
before every call and its error is RECORDED; the generator asserts only that it is below 1e-4.  It also asserts that the fp64
host mirror of this package (``_hostops.core_convolve`` per mode, unrounded) is within 1e-13 of every truth.  Only data is
written; no reference code is copied.
"""
import os
import sys

import numpy as np
import scipy.signal
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "convolve_f64.npz")
SEED = 41
PAIRS = [("p", "q"), ("q", "p"), ("v", "w"), ("m", "n"), ("k", "h"), ("p", "g")]
MODES = ("full", "same", "valid")


def rand_cores(shape, ranks, g):
    rs = [1] + list(ranks) + [1]
    return [torch.rand(rs[n], s, rs[n + 1], generator=g, dtype=torch.float64) for n, s in enumerate(shape)]


def dense(cores, Us):
    out = np.ones((1, 1))
    shape = []
    for c, U in zip(cores, Us):
        c = c.numpy()
        if U is not None:
            c = np.einsum("aib,ji->ajb", c, U.numpy())
        shape.append(c.shape[1])
        out = (out @ c.reshape(c.shape[0], -1)).reshape(-1, c.shape[2])
    return out.reshape(shape)


def window(I, J, mode):
    k, m = min(I, J), max(I, J)
    return {"full": (0, I + J - 1), "same": ((k - 1) // 2, m), "valid": (k - 1, m - k + 1)}[mode]


def reference_defined(sa, sb, mode):
    ks = [min(I, J) for I, J in zip(sa, sb)]
    if mode == "same":
        return all(k % 2 == 1 for k in ks)
    if mode == "valid":
        return all(k > 1 for k in ks)
    return True


def main(ref):
    sys.path.insert(0, ref)
    import tntorch as tn

    from tntorch_amd import _hostops

    g = torch.Generator().manual_seed(SEED)
    inputs = {
        "p": (rand_cores([5, 6, 7], [3, 3], g), [None] * 3),
        "q": (rand_cores([3, 4, 2], [2, 2], g), [None] * 3),
        "v": (rand_cores([4], [], g), [None]),
        "w": (rand_cores([4], [], g), [None]),
        "m": (rand_cores([5, 1, 4], [2, 2], g), [None] * 3),
        "n": (rand_cores([1, 6, 4], [2, 2], g), [None] * 3),
        "g": (rand_cores([3, 3, 3], [1, 1], g), [None] * 3),
        "k": (rand_cores([4, 5], [2], g), [torch.rand(6, 4, generator=g, dtype=torch.float64), None]),
        "h": (rand_cores([3, 2], [2], g), [None] * 2),
    }
    out = {}
    for name, (cores, Us) in inputs.items():
        out[name + "_ncores"] = np.array(len(cores))
        for n, c in enumerate(cores):
            out["{}_core{}".format(name, n)] = c.numpy()
            if Us[n] is not None:
                out["{}_U{}".format(name, n)] = Us[n].numpy()

    def T(name):
        cores, Us = inputs[name]
        return tn.Tensor([c.clone() for c in cores], Us=[None if U is None else U.clone() for U in Us])

    def absorbed(name):
        cores, Us = inputs[name]
        return [c if U is None else torch.einsum("aib,ji->ajb", c, U) for c, U in zip(cores, Us)]

    for a, b in PAIRS:
        da, db = dense(*inputs[a]), dense(*inputs[b])
        full = scipy.signal.convolve(da, db, mode="full", method="direct")
        for mode in MODES:
            case = "{}{}_{}".format(a, b, mode)
            wins = [window(I, J, mode) for I, J in zip(da.shape, db.shape)]
            truth = full[tuple(slice(lo, lo + K) for lo, K in wins)].copy()
            out["truth_" + case] = truth
            mirror = [_hostops.core_convolve(x, y, lo, K) for x, y, (lo, K) in zip(absorbed(a), absorbed(b), wins)]
            merr = np.linalg.norm(dense(mirror, [None] * len(mirror)) - truth) / np.linalg.norm(truth)
            assert merr < 1e-13, "{}: the fp64 mirror is {:.2e} off the truth".format(case, merr)
            if not reference_defined(da.shape, db.shape, mode):
                out["truthonly_" + case] = np.array(1)
                print("{:12s} shape {}  mirror {:.1e}  truth only".format(case, truth.shape, merr))
                continue
            torch.manual_seed(SEED)
            np.random.seed(SEED)
            res = tn.convolve(T(a), T(b), mode=mode, verbose=False).numpy()
            res = np.asarray(np.real(res), dtype=np.float64)
            assert res.shape == truth.shape, (case, res.shape, truth.shape)
            err = np.linalg.norm(res - truth) / np.linalg.norm(truth)
            print("{:12s} shape {}  mirror {:.1e}  reference error {:.2e}".format(case, truth.shape, merr, err))
            assert err < 1e-4, "{}: the reference is {:.2e} off the truth".format(case, err)
            out["ref_" + case], out["referr_" + case] = res, np.array(err)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

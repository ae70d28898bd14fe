"""Record tests/golden/completion_f64.npz from the unmodified reference's ``als_completion`` (tntorch; CPU, fp64, fixed seeds),
as tools/gen_cross_golden.py does for cross.

    python tools/gen_completion_golden.py /path/to/tntorch-checkout

Replay cases are ones where the reference is correct (its solution reshape only scrambles cores whose two ranks both exceed 1):
N = 2, and N = 3 with ranks_tt = [1, r].  Every slice holds more samples than unknowns and every system is of full rank.  One
case has weights, one is given x0, one draws x0 itself (x0 = None, seeded).  Samples are a low-rank TT plus a little noise.
Stored per case: X, y, (ws), the initial cores, the reference's cores and its values at the samples.

"rec4" is the evidence of the reference's bug: 4 modes of 10, an exact rank-3 target, 4000 random samples, 15 sweeps.  Stored:
the target cores, training / held-out samples and the reference's own training and held-out relative errors.
Only data is written; no reference code is copied.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "completion_f64.npz")

# name -> shape, TT ranks of the sample generator, ranks_tt of the call, P, niter, weighted, x0 given (else drawn by the call)
CASES = {
    "n2": ([8, 9], [3], 3, 200, 4, False, False),
    "n2w": ([10, 12], [2], 2, 300, 4, True, False),
    "n3x0": ([6, 7, 8], [1, 3], [1, 3], 400, 4, False, True),
    "n3": ([5, 6, 7], [1, 2], [1, 2], 300, 3, False, False),
}


def tt_cores(shape, ranks, g):
    rs = [1] + list(ranks) + [1]
    return [torch.randn(rs[n], shape[n], rs[n + 1], generator=g) for n in range(len(shape))]


def tt_values(cores, X):
    v = torch.ones(X.shape[0], 1, dtype=torch.float64)
    for n, c in enumerate(cores):
        v = torch.einsum("pa,apb->pb", v, c[:, X[:, n], :])
    return v[:, 0]


def samples(shape, P, g):
    """P random positions that cover every slice more than 3 times over (resampled until they do)."""
    while True:
        X = torch.stack([torch.randint(0, s, (P,), generator=g) for s in shape], dim=1)
        if all(torch.bincount(X[:, n], minlength=s).min() > 3 for n, s in enumerate(shape)):
            return X


def main(ref):
    sys.path.insert(0, ref)
    import tntorch as tn

    torch.set_default_dtype(torch.float64)
    out = {"cases": np.array(list(CASES))}
    for k, (name, (shape, gen_ranks, ranks_tt, P, niter, weighted, given)) in enumerate(CASES.items()):
        g = torch.Generator().manual_seed(1000 + k)
        X = samples(shape, P, g)
        y = tt_values(tt_cores(shape, gen_ranks, g), X) + 1e-3 * torch.randn(P, generator=g)
        ws = (0.5 + torch.rand(P, generator=g)) if weighted else None
        seed = 10 + k
        torch.manual_seed(seed)
        x0 = tn.rand(shape, ranks_tt=ranks_tt)
        init = [c.clone() for c in x0.cores]
        torch.manual_seed(seed)
        t = tn.als_completion(X, y, ranks_tt=ranks_tt, ws=ws, x0=x0 if given else None, niter=niter, verbose=False)
        out[name + "_X"] = X.numpy()
        out[name + "_y"] = y.numpy()
        if weighted:
            out[name + "_ws"] = ws.numpy()
        out[name + "_meta"] = np.array([seed, niter, int(given)] + list(np.atleast_1d(ranks_tt)) + [0] * (3 - len(np.atleast_1d(ranks_tt))))
        for n, c in enumerate(init):
            out["{}_init{}".format(name, n)] = c.numpy()
        for n, c in enumerate(t.cores):
            out["{}_core{}".format(name, n)] = c.numpy()
        out[name + "_values"] = t[X].torch().numpy()
        print(name, "ranks", t.ranks_tt.tolist(), "fit", float(torch.norm(t[X].torch() - y) / torch.norm(y)))

    # the 4-mode exact rank-3 case: the reference's own errors
    g = torch.Generator().manual_seed(77)
    target = tt_cores([10] * 4, [3, 3, 3], g)
    X = torch.stack([torch.randint(0, 10, (4000,), generator=g) for _ in range(4)], dim=1)
    Xh = torch.stack([torch.randint(0, 10, (1000,), generator=g) for _ in range(4)], dim=1)
    y, yh = tt_values(target, X), tt_values(target, Xh)
    torch.manual_seed(5)
    t = tn.als_completion(X, y, ranks_tt=3, niter=15, verbose=False)
    err = float(torch.norm(t[X].torch() - y) / torch.norm(y))
    err_h = float(torch.norm(t[Xh].torch() - yh) / torch.norm(yh))
    for n, c in enumerate(target):
        out["rec4_target{}".format(n)] = c.numpy()
    out["rec4_X"], out["rec4_Xh"] = X.numpy(), Xh.numpy()
    out["rec4_ref_err"] = np.array([err, err_h])
    out["rec4_seed"], out["rec4_niter"] = np.array(5), np.array(15)
    print("rec4 reference training / held-out error", err, err_h)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

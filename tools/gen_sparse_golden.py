"""Record tests/golden/sparse_tt_svd_f64.npz from the unmodified reference's ``sparse_tt_svd`` (tntorch; CPU, fp64, fixed seed),
as tools/gen_completion_golden.py does for als_completion.

    python tools/gen_sparse_golden.py /path/to/tntorch-checkout

Cases (a 6x5x7x4 tensor from a rank-(3,3,2) train unless noted):
  dense   every position, in shuffled order (dense as sparse), eps = 1e-6
  s200    200 distinct random positions, eps = 0.2
  s200r   the same 200 positions, eps = 1e-9, rmax = 4
  n2      a 9x8 matrix of rank 3, 40 distinct random positions, eps = 1e-3
Stored per case: X, y, eps, rmax (0 = none), the reference's ranks and its dense reconstruction.

Two things are asserted for every case, by a dense re-computation of the steps with numpy's SVD at the reference's ranks: the
reference's ranks lie within the column cap of tntorch_amd (the number of non-zero columns of every unfolding), and no tail
energy that the rank rule compares lies within a relative 1e-6 of delta^2 (the rank decisions do not hinge on rounding).
Pick another seed when either fails.  Only data is written; no reference code is copied.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "sparse_tt_svd_f64.npz")
SEED = 7

# name -> shape, TT ranks of the generator, number of positions (0: all), eps, rmax (0: none)
CASES = {
    "dense": ([6, 5, 7, 4], [3, 3, 2], 0, 1e-6, 0),
    "s200": ([6, 5, 7, 4], [3, 3, 2], 200, 0.2, 0),
    "s200r": ([6, 5, 7, 4], [3, 3, 2], 200, 1e-9, 4),
    "n2": ([9, 8], [3], 40, 1e-3, 0),
}


def tt_dense(shape, ranks, g):
    rs = [1] + list(ranks) + [1]
    out = torch.ones(1, 1, dtype=torch.float64)
    for n, s in enumerate(shape):
        core = torch.randn(rs[n], s, rs[n + 1], generator=g, dtype=torch.float64)
        out = (out @ core.reshape(rs[n], -1)).reshape(-1, rs[n + 1])
    return out.reshape(shape)


def check_steps(full, ranks, eps, norm_y):
    """Dense TT-SVD steps at the given ranks: the column cap and the distance of every tail energy from delta^2."""
    N = full.dim()
    delta2 = (eps / np.sqrt(N - 1) * norm_y) ** 2
    M = full.numpy().reshape(full.shape[0], -1)
    for n in range(N - 1):
        cols = int((np.abs(M).sum(axis=0) > 0).sum())
        assert ranks[n + 1] <= cols, "rank {} of bond {} above the column cap {}".format(ranks[n + 1], n + 1, cols)
        u, s, _ = np.linalg.svd(M, full_matrices=False)
        tails = np.cumsum((s**2)[::-1])
        live = tails[tails > 1e-24 * tails[-1]]  # (tail energies of numerically null directions lie far below any delta^2 here)
        assert np.all(np.abs(live - delta2) > 1e-6 * delta2), "a tail energy of bond {} lies at delta^2".format(n + 1)
        q = ranks[n + 1]
        M = (u[:, :q].T @ M).reshape(q * full.shape[n + 1], -1)


def main(ref):
    sys.path.insert(0, ref)
    import tntorch as tn

    torch.set_default_dtype(torch.float64)
    g = torch.Generator().manual_seed(SEED)
    out = {"cases": np.array(list(CASES))}
    full, picks = {}, {}
    for name, (shape, gen_ranks, P, eps, rmax) in CASES.items():
        key = (tuple(shape), P)
        if tuple(shape) not in full:
            full[tuple(shape)] = tt_dense(shape, gen_ranks, g)
        if key not in picks:  # distinct positions in shuffled order (s200 and s200r share theirs)
            total = int(np.prod(shape))
            flat = torch.randperm(total, generator=g)[: P or total]
            picks[key] = torch.stack(torch.unravel_index(flat, shape), dim=1)
        X = picks[key]
        y = full[tuple(shape)][tuple(X.t())]
        t = tn.sparse_tt_svd(X.clone(), y.clone(), eps, rmax=rmax or None)
        ranks = [int(r) for r in t.ranks_tt]
        sparse = torch.zeros(shape, dtype=torch.float64)
        sparse[tuple(X.t())] = y
        check_steps(sparse, ranks, eps, float(torch.norm(y)))
        recon = t.torch()
        out[name + "_X"], out[name + "_y"] = X.numpy(), y.numpy()
        out[name + "_eps"], out[name + "_rmax"] = np.array(eps), np.array(rmax)
        out[name + "_ranks"], out[name + "_recon"] = np.array(ranks), recon.numpy()
        print(name, "ranks", ranks, "error against the zero-filled tensor", float(torch.norm(recon - sparse) / torch.norm(sparse)))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

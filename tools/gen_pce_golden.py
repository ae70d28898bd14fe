"""Record tests/golden/pce_f64.npz from the unmodified reference's ``PCEInterpolator`` and its helpers (tntorch; CPU, fp64, fixed
seed), as tools/gen_sparse_golden.py does for sparse_tt_svd.  Needs scikit-learn (the reference's ``fit`` imports it).

    python tools/gen_pce_golden.py /path/to/tntorch-checkout

The reference's ``fit`` still spells ``np.int``; this process sets ``np.int = int`` before calling it, and an fp64 default dtype
(the reference casts through ``torch.Tensor``).  Its ``empirical_marginals`` calls a ``tn.discretize`` that does not exist and is
not recorded.

Stored:
  X [300, 3], y     noisy samples of a smooth function on the box [0, 2] x [-1, 3] x [5, 6]; seed, p, q, val_split of ``fit``
  Psis, allcoords, coords, coef, X_mean, X_std, bbox                          what ``fit`` leaves behind
  Xtest [50, 3], ytest                                                        ``predict`` at held-out points
  dense                                                                       ``to_tensor(domain=8, eps=1e-10).torch()``
  gs_uniform, gs_normal [500], gs_uniform_Psi, gs_normal_Psi [6, 6]           ``gram_schmidt(x, 6)`` on standardised samples
  h_X [12, 3], h_bbox, h_idx, h_idx16, h_domain_<n>, h_idx_domain, h_feat, h_feat_domain
      ``get_bounding_box`` / ``features2indices`` / ``indices2features`` on a small matrix, with and without ``domain``
Only data is written; no reference code is copied.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "pce_f64.npz")
SEED = 11
P, PTEST, FIT = 300, 50, dict(p=4, q=0.75, val_split=0.1, seed=3)
LO, HI = np.array([0.0, -1.0, 5.0]), np.array([2.0, 3.0, 6.0])
GS_P, GS_S = 500, 6


def target(X):
    u = (X - LO) / (HI - LO)
    return np.sin(2.0 * u[:, 0]) + u[:, 1] * u[:, 2] + 0.5 * u[:, 0] ** 2 * u[:, 2] - u[:, 1] ** 3


def main(ref):
    sys.path.insert(0, ref)
    np.int = int
    import tntorch as tn

    torch.set_default_dtype(torch.float64)
    rng = np.random.default_rng(SEED)
    X = rng.uniform(LO, HI, (P, 3))
    y = target(X) + 0.05 * rng.standard_normal(P)
    Xtest = rng.uniform(LO, HI, (PTEST, 3))
    out = {"X": X, "y": y, "Xtest": Xtest}
    out.update({k: np.array(v) for k, v in FIT.items()})

    m = tn.PCEInterpolator()
    m.fit(torch.tensor(X), torch.tensor(y), retrain=True, verbose=False, **FIT)
    out["Psis"] = torch.stack(m.Psis).numpy()
    out["allcoords"], out["coords"], out["coef"] = m.allcoords.numpy(), m.coords.numpy(), m.coef.numpy()
    out["X_mean"], out["X_std"], out["bbox"] = m.X_mean.numpy(), m.X_std.numpy(), np.array(m.bbox)
    out["ytest"] = m.predict(torch.tensor(Xtest)).numpy()
    out["dense"] = m.to_tensor(domain=8, eps=1e-10, verbose=False).torch().numpy()
    print("candidates", len(m.allcoords), "selected", len(m.coords), "dense", out["dense"].shape)

    for name, x in (("uniform", rng.uniform(-1.0, 1.0, GS_P)), ("normal", rng.standard_normal(GS_P))):
        x = (x - x.mean()) / x.std(ddof=1)
        out["gs_" + name] = x
        out["gs_" + name + "_Psi"] = tn.gram_schmidt(torch.tensor(x), GS_S).numpy()

    hX = rng.uniform(LO, HI, (12, 3))
    domain = [torch.tensor(np.sort(rng.uniform(LO[n], HI[n], 9))) for n in range(3)]
    hbbox = tn.get_bounding_box(torch.tensor(hX))
    out["h_X"], out["h_bbox"] = hX, np.array(hbbox)
    out["h_idx"] = tn.features2indices(torch.tensor(hX)).numpy()
    out["h_idx16"] = tn.features2indices(torch.tensor(hX), bbox=[(LO[n] + 0.3, HI[n] - 0.2) for n in range(3)], I=16).numpy()
    out["h_idx_domain"] = tn.features2indices(torch.tensor(hX), domain=domain).numpy()
    for n in range(3):
        out["h_domain_{}".format(n)] = domain[n].numpy()
    out["h_feat"] = tn.indices2features(torch.tensor(out["h_idx16"]), bbox=hbbox, I=16).numpy()
    out["h_feat_domain"] = tn.indices2features(torch.tensor(out["h_idx_domain"]), domain=domain).numpy()

    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

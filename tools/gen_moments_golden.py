"""Record tests/golden/moments_f32.npz from the unmodified reference's moment family (tntorch ``metrics.py``: ``hadamard_sum``,
``raw_moment``, ``normalized_moment``, ``var``, ``std``; CPU, fixed seed), as tools/gen_sparse_golden.py does for sparse_tt_svd.

    python tools/gen_moments_golden.py /path/to/tntorch-checkout

The reference creates its intermediates in the default dtype, so it only runs in fp32: the fixtures are fp32.  All cores are drawn
with ``rand`` (positive entries: sums of positive terms are well conditioned, which keeps the comparison with the truth
meaningful).  Inputs (their cores are stored):
  a     5x6x7x4, TT ranks 3          b     5x6x7x4, TT ranks 2
  v     a one-mode tensor (6)        m     a 4x4 matrix of rank 2
  marg  one set of (positive, unnormalised) marginals for the 5x6x7x4 shape
Stored per quantity q: ``ref_q`` (the reference's value, NaN where the reference has none) and ``truth_q`` (the same quantity
computed densely in fp64 with numpy from the stored cores):
  hsum_exact_M1..M4        hadamard_sum of [a], [a, b], [a, b, a], [a, b, a, b], algorithm "exact"
  hsum_eig_M3, hsum_svd_M3 hadamard_sum([a, b, a], eps = 1e-6)
  raw_k1..k4, rawm_k1..k4  raw_moment(a, k) without / with the marginals (the reference's defaults: "eig", eps = 1e-6)
  norm_k3, norm_k4         normalized_moment(a, k) (defaults: "eig", eps = 1e-12)
  var, varm, std           var(a), var(a, marg), std(a)
  v_hsum_exact_M3          hadamard_sum([v, v, v]) ("exact"; the reference's approximate path returns None for one mode)
  m_raw_k3                 raw_moment(m, 3)
The generator asserts that every value of the reference lies within a relative 1e-5 of the truth (pick another seed if not) and
prints, per quantity, the reference's error and the ratio prod_m ||t_m||_M / |sum| of the Hadamard sum behind it (the Hoelder
bound over the value: how much cancellation the sum hides), and the largest such ratio at the end.  Only data is written; no
reference code is copied.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "moments_f32.npz")
SEED = 11


def rand_cores(shape, ranks, g):
    rs = [1] + list(ranks) + [1]
    return [torch.rand(rs[n], s, rs[n + 1], generator=g, dtype=torch.float32) for n, s in enumerate(shape)]


def dense(cores):
    out = np.ones((1, 1))
    for c in cores:
        c = c.double().numpy()
        out = (out @ c.reshape(c.shape[0], -1)).reshape(-1, c.shape[2])
    return out.reshape([c.shape[1] for c in cores])


def holder_ratio(ds):
    """prod_m ||t_m||_M / |sum(prod_m t_m)| for dense operands ds."""
    M = len(ds)
    val = np.prod(np.stack(ds), axis=0).sum()
    return float(np.prod([(np.abs(d) ** M).sum() ** (1.0 / M) for d in ds]) / abs(val))


def main(ref):
    sys.path.insert(0, ref)
    import tntorch as tn

    g = torch.Generator().manual_seed(SEED)
    shape = [5, 6, 7, 4]
    ca, cb = rand_cores(shape, [3, 3, 3], g), rand_cores(shape, [2, 2, 2], g)
    cv, cm = rand_cores([6], [], g), rand_cores([4, 4], [2], g)
    marg = [torch.rand(s, generator=g, dtype=torch.float32) + 0.1 for s in shape]
    out = {}
    for name, cores in (("a", ca), ("b", cb), ("v", cv), ("m", cm)):
        out[name + "_ncores"] = np.array(len(cores))
        for n, c in enumerate(cores):
            out["{}_core{}".format(name, n)] = c.numpy()
    for n, w in enumerate(marg):
        out["marg{}".format(n)] = w.numpy()

    def T(cores):
        return tn.Tensor([c.clone() for c in cores])

    a, b, v, m = dense(ca), dense(cb), dense(cv), dense(cm)
    w = [x.double().numpy() / x.double().numpy().sum() for x in marg]
    pdf = np.einsum("i,j,k,l->ijkl", *w)
    mean, meanm = a.mean(), (a * pdf).sum()
    ac, acm = a - mean, a - meanm
    var = (ac**2).mean()
    worst = 0.0

    def record(name, ref_value, truth, operands):
        nonlocal worst
        out["truth_" + name] = np.array(truth, dtype=np.float64)
        out["ref_" + name] = np.array(np.nan if ref_value is None else float(ref_value), dtype=np.float64)
        ratio = holder_ratio(operands)
        worst = max(worst, ratio)
        if ref_value is None:
            print("{:18s} truth {:.10g}  (no reference value)  ratio {:.3g}".format(name, truth, ratio))
            return
        err = abs(float(ref_value) - truth) / abs(truth)
        print("{:18s} truth {:.10g}  reference {:.10g}  rel. error {:.2e}  ratio {:.3g}".format(name, truth, float(ref_value), err, ratio))
        assert err < 1e-5, "{}: the reference is {:.2e} off the truth; pick another seed".format(name, err)

    lists = {1: [(ca, a)], 2: [(ca, a), (cb, b)], 3: [(ca, a), (cb, b), (ca, a)], 4: [(ca, a), (cb, b), (ca, a), (cb, b)]}
    for M, ops in lists.items():
        ds = [d for _, d in ops]
        record("hsum_exact_M{}".format(M), tn.hadamard_sum([T(c) for c, _ in ops], algorithm="exact"), np.prod(np.stack(ds), axis=0).sum(), ds)
    ds = [d for _, d in lists[3]]
    for alg in ("eig", "svd"):
        record("hsum_{}_M3".format(alg), tn.hadamard_sum([T(c) for c, _ in lists[3]], algorithm=alg, eps=1e-6),
               np.prod(np.stack(ds), axis=0).sum(), ds)
    for k in range(1, 5):
        record("raw_k{}".format(k), tn.raw_moment(T(ca), k), (a**k).mean(), [a] * k)
        record("rawm_k{}".format(k), tn.raw_moment(T(ca), k, marginals=[x.clone() for x in marg]), (a**k * pdf).sum(), [a] * (k - 1) + [a * pdf])
    for k in (3, 4):
        record("norm_k{}".format(k), tn.normalized_moment(T(ca), k), (ac**k).mean() / var ** (k / 2.0), [ac] * k)
    record("var", tn.var(T(ca)), var, [ac, ac])
    record("varm", tn.var(T(ca), marginals=[x.clone() for x in marg]), (acm**2 * pdf).sum(), [acm * pdf, acm])
    record("std", tn.std(T(ca)), np.sqrt(var), [ac, ac])
    record("v_hsum_exact_M3", tn.hadamard_sum([T(cv)] * 3, algorithm="exact"), (v**3).sum(), [v] * 3)
    record("m_raw_k3", tn.raw_moment(T(cm), 3), (m**3).mean(), [m] * 3)
    print("largest ratio ||operands|| / |value|: {:.4g}".format(worst))
    out["largest_ratio"] = np.array(worst)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

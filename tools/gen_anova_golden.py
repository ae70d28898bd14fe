"""Record tests/golden/anova_f64.npz from the unmodified reference's ``anova.py`` (``anova_decomposition``,
``undo_anova_decomposition``, ``truncate_anova``, ``sobol``, ``mean_dimension``, ``dimension_distribution``; CPU, fp64 inputs, fixed
seed), as tools/gen_derivatives_golden.py does for the differential operators.

    python tools/gen_anova_golden.py /path/to/tntorch-checkout

All cores are drawn with ``rand`` in fp64.  Inputs (their cores are stored):
  t           3x4x5x3, TT ranks 3
  k           a 6x5 Tucker-TT: core modes 4x5, TT rank 2, one factor [6, 4] on mode 0
  marg0..3    positive, unnormalised marginals for the shape of t;  kmarg0..1  the same for k
  mask_<m>    the cores of the reference's masks over 4 variables (x = tn.symbols(4)):
              only_x0 = only(x0), x0, x0_not_x2 = x0 & ~x2, weight = weight(4), one_hot = weight_one_hot(4, 5), true = true(4);
              kmask_x0 = x0 over the 2 variables of k
Stored per quantity q: ``ref_q`` (the reference's result) and ``truth_q``, from a dense brute-force ANOVA in fp64 numpy: the terms
f_u = sum_{v <= u} (-1)^(|u| - |v|) E[f | x_v] of every subset u of the variables, their variances D_u = E[f_u^2] under the
normalised marginals, and for a mask m (a 2^N table, vector-valued where its last rank is above 1)
sum_{u != {}} m[u] D_u, divided by sum_{u != {}} D_u where normalised:
  sobol_<m>, sobol_<m>_raw          sobol(t, mask_<m>, marg), normalize on / off
  sobol_uniform_x0                  sobol(t, x0): default (uniform) marginals
  mean_dimension, mean_dimension_x0 mean_dimension(t, marginals=marg), and with mask = x0
  dimdist, dimdist_o2, dimdist_x0, dimdist_x0_o2   dimension_distribution(t, marginals=marg), with order = 2, mask = x0, both
  ksobol_x0, ksobol_x0_raw, kmean_dimension        the Tucker input
  truncate_only_x1                  truncate_anova(t, only(x1)), uniform marginals: one-mode, the first-order term of x1 (only(x1)
                                    does not accept the empty tuple: the mean is cut with every other term);
                                    truncate_only_x1_keepdim the same with keepdim=True (the shape of t), truncate_only_x1_marg
                                    with marginals=marg
  truncate_only_x1_or_none[_marg]   truncate_anova(t, only(x1) | none(4)): the mean plus the first-order term of x1
  var_terms (truth only)            D_u of t under marg for the 16 subsets, u as the bits of the index (bit n = variable n)
The generator asserts: every reference result within 1e-10 of the truth (absolute; the indices lie in [0, N]), the tensor-valued
ones relative to the truth's largest entry; the reference's extended tensor has factors of I + 1 rows and idxs [0] + [1] * I, and
undoes to t within 1e-12.  Only data is written; no reference code is copied.
"""
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "anova_f64.npz")
SEED = 41


def rand_cores(shape, ranks, g):
    rs = [1] + list(ranks) + [1]
    return [torch.rand(rs[n], s, rs[n + 1], generator=g, dtype=torch.float64) for n, s in enumerate(shape)]


def dense(cores, Us=None, keep_last=False):
    """The dense tensor of a train; with ``keep_last`` the trailing rank stays as one more axis."""
    out = np.ones((1, cores[0].shape[0]))
    shape = []
    for n, c in enumerate(cores):
        c = c.numpy()
        if Us is not None and Us[n] is not None:
            c = np.einsum("aib,ji->ajb", c, Us[n].numpy())
        shape.append(c.shape[1])
        out = (out @ c.reshape(c.shape[0], -1)).reshape(-1, c.shape[2])
    if keep_last:
        return out.reshape(shape + [out.shape[1]])
    return out.sum(axis=1).reshape(shape)


def anova_terms(f, ws):
    """{u (tuple of 0/1 per variable): f_u, broadcastable to f} of the dense tensor f under the weights ws (each sums to 1)."""
    N = f.ndim
    cond = {}
    for u in itertools.product((0, 1), repeat=N):   # E[f | x_u]: the other variables integrated out
        e = f
        for n in range(N):
            if not u[n]:
                e = np.tensordot(e, ws[n], axes=(n, 0))
                e = np.expand_dims(e, n)
        cond[u] = e
    terms = {}
    for u in itertools.product((0, 1), repeat=N):
        acc = 0.0
        for v in itertools.product((0, 1), repeat=N):
            if all(v[n] <= u[n] for n in range(N)):
                acc = acc + (-1.0) ** (sum(u) - sum(v)) * cond[v]
        terms[u] = acc
    return terms


def variances(f, ws):
    """{u: D_u}."""
    out = {}
    for u, fu in anova_terms(f, ws).items():
        x = np.broadcast_to(fu, f.shape) ** 2
        for n in range(f.ndim - 1, -1, -1):
            x = np.tensordot(x, ws[n], axes=(n, 0))
        out[u] = float(x)
    return out


def selected(D, m, normalize):
    """sum_{u != {}} m[u] D_u (m a 2^N table, or [2, .., 2, S]), over the total variance where ``normalize``."""
    num = sum(m[u] * D[u] for u in D if any(u))
    den = sum(D[u] for u in D if any(u))
    return np.asarray(num / den if normalize else num, dtype=np.float64)


def main(ref):
    sys.path.insert(0, ref)
    import tntorch as tn

    # the reference builds its masks, default marginals and the closing identity core of the one-hot case in torch's default
    # dtype, and its dot refuses mixed dtypes: with fp64 inputs the default has to be fp64
    torch.set_default_dtype(torch.float64)
    g = torch.Generator().manual_seed(SEED)
    ct = rand_cores([3, 4, 5, 3], [3, 3, 3], g)
    ck = rand_cores([4, 5], [2], g)
    uk = [torch.rand(6, 4, generator=g, dtype=torch.float64), None]
    marg = [torch.rand(s, generator=g, dtype=torch.float64) + 0.1 for s in [3, 4, 5, 3]]
    kmarg = [torch.rand(s, generator=g, dtype=torch.float64) + 0.1 for s in [6, 5]]
    out = {}
    for name, cores in (("t", ct), ("k", ck)):
        out[name + "_ncores"] = np.array(len(cores))
        for n, c in enumerate(cores):
            out["{}_core{}".format(name, n)] = c.numpy()
    out["k_U0"] = uk[0].numpy()
    for n, w in enumerate(marg):
        out["marg{}".format(n)] = w.numpy()
    for n, w in enumerate(kmarg):
        out["kmarg{}".format(n)] = w.numpy()

    def T(cores, Us=None):
        return tn.Tensor([c.clone() for c in cores], Us=None if Us is None else [None if U is None else U.clone() for U in Us])

    def margs(ms):
        return [m.clone() for m in ms]   # the reference normalises the vectors it is given in place

    x = tn.symbols(4)
    masks = {"only_x0": tn.only(x[0]), "x0": x[0], "x0_not_x2": x[0] & ~x[2], "weight": tn.weight(4),
             "one_hot": tn.weight_one_hot(4, 5), "true": tn.true(4)}
    kmasks = {"x0": tn.symbols(2)[0]}
    tables = {}
    for prefix, ms in (("mask_", masks), ("kmask_", kmasks)):
        for name, m in ms.items():
            assert all(U is None for U in m.Us) and all(c.dim() == 3 for c in m.cores)
            cores = [c.double() for c in m.cores]
            out["{}{}_ncores".format(prefix, name)] = np.array(len(cores))
            for n, c in enumerate(cores):
                out["{}{}_core{}".format(prefix, name, n)] = c.numpy()
            table = dense(cores, keep_last=True)
            tables[prefix + name] = table[..., 0] if table.shape[-1] == 1 else table

    def record(name, ref_value, truth, relative=False, bound=1e-10):
        ref_value = np.asarray(ref_value, dtype=np.float64)
        truth = np.asarray(truth, dtype=np.float64)
        assert ref_value.shape == truth.shape, (name, ref_value.shape, truth.shape)
        err = np.abs(ref_value - truth).max() / (np.abs(truth).max() if relative else 1.0)
        print("{:28s} max |truth| {:.6g}  reference error {:.2e}".format(name, np.abs(truth).max(), err))
        assert err < bound, "{}: the reference is {:.2e} off the truth".format(name, err)
        out["truth_" + name], out["ref_" + name] = truth, ref_value

    def value(r):
        return r.numpy() if hasattr(r, "cores") else r.detach().numpy()

    t, k = dense(ct), dense(ck, uk)
    ws = [(m / m.sum()).numpy() for m in marg]
    kws = [(m / m.sum()).numpy() for m in kmarg]
    uni = [np.full(s, 1.0 / s) for s in t.shape]
    D, Dk, Du = variances(t, ws), variances(k, kws), variances(t, uni)
    out["truth_var_terms"] = np.array([D[tuple((j >> n) & 1 for n in range(4))] for j in range(16)])
    print("variances of the ANOVA terms of t:", out["truth_var_terms"])

    for name, m in masks.items():
        for norm, suffix in ((True, ""), (False, "_raw")):
            record("sobol_{}{}".format(name, suffix), value(tn.sobol(T(ct), m, margs(marg), normalize=norm)),
                   selected(D, tables["mask_" + name], norm))
    record("sobol_uniform_x0", value(tn.sobol(T(ct), masks["x0"])), selected(Du, tables["mask_x0"], True))
    record("mean_dimension", value(tn.mean_dimension(T(ct), marginals=margs(marg))), selected(D, tables["mask_weight"], True))
    record("mean_dimension_x0", value(tn.mean_dimension(T(ct), mask=masks["x0"], marginals=margs(marg))),
           selected(D, tables["mask_weight"] * tables["mask_x0"], True) / selected(D, tables["mask_x0"], True))
    oh = tables["mask_one_hot"]
    record("dimdist", value(tn.dimension_distribution(T(ct), marginals=margs(marg))), selected(D, oh, True)[1:])
    record("dimdist_o2", value(tn.dimension_distribution(T(ct), order=2, marginals=margs(marg))), selected(D, oh[..., :3], True)[1:])
    x0 = tables["mask_x0"]
    record("dimdist_x0", value(tn.dimension_distribution(T(ct), mask=masks["x0"], marginals=margs(marg))),
           selected(D, oh * x0[..., None], True)[1:] / selected(D, x0, True))
    record("dimdist_x0_o2", value(tn.dimension_distribution(T(ct), mask=masks["x0"], order=2, marginals=margs(marg))),
           selected(D, oh[..., :3] * x0[..., None], True)[1:] / selected(D, x0, True))
    for norm, suffix in ((True, ""), (False, "_raw")):
        record("ksobol_x0" + suffix, value(tn.sobol(T(ck, uk), kmasks["x0"], margs(kmarg), normalize=norm)),
               selected(Dk, tables["kmask_x0"], norm))
    record("kmean_dimension", value(tn.mean_dimension(T(ck, uk), marginals=margs(kmarg))),
           selected(Dk, dense([c.double() for c in tn.weight(2).cores]), True))

    x1 = tn.only(x[1])
    for name, w, kw in (("truncate_only_x1", uni, {}), ("truncate_only_x1_marg", ws, {"marginals": margs(marg)})):
        terms = anova_terms(t, w)
        res = tn.truncate_anova(T(ct), x1, keepdim=False, **kw)
        assert res.dim() == 1
        record(name, res.numpy(), terms[(0, 1, 0, 0)].reshape(-1), relative=True)
        res = tn.truncate_anova(T(ct), x1 | tn.none(4), keepdim=False, **kw)
        assert res.dim() == 1
        record(name.replace("only_x1", "only_x1_or_none"), res.numpy(), (terms[(0, 0, 0, 0)] + terms[(0, 1, 0, 0)]).reshape(-1),
               relative=True)
    res = tn.truncate_anova(T(ct), x1, keepdim=True)
    terms = anova_terms(t, uni)
    record("truncate_only_x1_keepdim", res.numpy(), np.broadcast_to(terms[(0, 1, 0, 0)], t.shape).copy(),
           relative=True)

    for cores, Us, full in ((ct, None, t), (ck, uk, k)):
        a = tn.anova_decomposition(T(cores, Us))
        assert [tuple(U.shape) for U in a.Us] == [(I + 1, I if Us is None or Us[n] is None else Us[n].shape[1])
                                                  for n, I in enumerate(full.shape)]
        assert [list(np.asarray(i)) for i in a.idxs] == [[0] + [1] * I for I in full.shape]
        back = tn.undo_anova_decomposition(a).numpy()
        assert np.abs(back - full).max() <= 1e-12 * np.abs(full).max()
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

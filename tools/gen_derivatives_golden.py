"""Record tests/golden/derivatives_f64.npz from the unmodified reference's ``derivatives.py`` (``partial``, ``gradient``,
``laplacian``, ``divergence``, ``curl``, ``dgsm``, ``active_subspace``; CPU, fp64 inputs, fixed seed), as
tools/gen_moments_golden.py does for the moment family.

    python tools/gen_derivatives_golden.py /path/to/tntorch-checkout

All cores are drawn with ``rand`` in fp64.  Inputs (their cores are stored):
  a           5x6x7x4, TT ranks 3                       v   a one-mode tensor (6)
  f0, f1, f2  5x5x5, TT ranks (3, 2): a vector field     k   a 6x5 Tucker-TT: core modes 4x5, TT rank 2, one factor [6, 4] on mode 0
  bnd_a / bnd_f / bnd_k / bnd_v   explicit bounds, one pair per mode
  marg0..3    positive, unnormalised marginals for the shape of a
Every call passes explicit bounds, or (``partial_f0_default``) uses equal mode sizes with dim = 0, so that the reference's way of
indexing its default bounds by the position in ``dim`` never enters.  Stored per quantity q: ``ref_q`` (the reference's result,
densified) and ``truth_q`` (computed densely in fp64 numpy from the stored cores with the matrix S / step of derivatives.py:96-129):
  partial_a_d{0,1,3}_o{1,2,3}_p{0,1}   partial(a, d, order=o, bounds=bnd_a[d], periodic=p): a first, a middle and the last mode
  partial_k_d0_o{1,2,3}_p{0,1}         the same on the Tucker factor of k
  partial_v_o1, partial_f0_default     the one-mode tensor; partial(f0, 0) with default bounds
  gradient_a_{0..3}                    gradient(a, bounds=bnd_a)
  laplacian_a, laplacian_f0, laplacian_k, laplacian_v
  divergence_f, curl_f_{0,1,2}         of [f0, f1, f2] with bnd_f
  dgsm_a                               dgsm(a, bnd_a, marg)
  as_M (truth only), as_w, as_v        active_subspace(a, bnd_a, marg): the matrix, eigenvalues (descending) and eigenvectors
The generator asserts: every tensor-valued reference result within 1e-12 of the truth, relative to the truth's largest entry;
``dgsm`` / ``active_subspace`` within 1e-5 (the reference keeps those in fp32); the active-subspace eigenvalues separated by at
least 10 % of the largest (pick another seed if not).  Only data is written; no reference code is copied.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "derivatives_f64.npz")
SEED = 32


def rand_cores(shape, ranks, g):
    rs = [1] + list(ranks) + [1]
    return [torch.rand(rs[n], s, rs[n + 1], generator=g, dtype=torch.float64) for n, s in enumerate(shape)]


def dense(cores, Us=None):
    out = np.ones((1, 1))
    for n, c in enumerate(cores):
        c = c.numpy()
        if Us is not None and Us[n] is not None:
            c = np.einsum("aib,ji->ajb", c, Us[n].numpy())
        out = (out @ c.reshape(c.shape[0], -1)).reshape(-1, c.shape[2])
    return out.reshape([c.shape[1] if Us is None or Us[n] is None else Us[n].shape[0] for n, c in enumerate(cores)])


def stencil(I, b, periodic=False):
    """S / step of derivatives.py:96-129 for a mode of size I with bounds b."""
    S = np.zeros((I, I))
    if periodic:
        for i in range(I):
            S[i, (i + 1) % I] += 1.0
            S[i, (i - 1) % I] -= 1.0
    elif I > 1:
        for i in range(1, I - 1):
            S[i, i + 1], S[i, i - 1] = 1.0, -1.0
        S[0, 1] += 2.0
        S[0, 0] -= 2.0
        S[I - 1, I - 1] += 2.0
        S[I - 1, I - 2] -= 2.0
    return S / ((b[1] - b[0]) / (I + 1) * 2)


def along(x, d, Mx):
    return np.moveaxis(np.tensordot(Mx, x, axes=(1, d)), 0, d)


def main(ref):
    sys.path.insert(0, ref)
    import tntorch as tn

    g = torch.Generator().manual_seed(SEED)
    ca = rand_cores([5, 6, 7, 4], [3, 3, 3], g)
    cf = [rand_cores([5, 5, 5], [3, 2], g) for _ in range(3)]
    cv = rand_cores([6], [], g)
    ck = rand_cores([4, 5], [2], g)
    uk = [torch.rand(6, 4, generator=g, dtype=torch.float64), None]
    marg = [torch.rand(s, generator=g, dtype=torch.float64) + 0.1 for s in [5, 6, 7, 4]]
    bnd = {"a": [[0.0, 3.0], [0.0, 2.0], [0.0, 1.5], [0.0, 1.0]], "f": [[0.0, 2.0], [-1.0, 1.0], [0.0, 5.0]],
           "k": [[0.0, 2.5], [1.0, 3.0]], "v": [[-2.0, 2.0]]}
    out = {}
    for name, cores in (("a", ca), ("f0", cf[0]), ("f1", cf[1]), ("f2", cf[2]), ("v", cv), ("k", ck)):
        out[name + "_ncores"] = np.array(len(cores))
        for n, c in enumerate(cores):
            out["{}_core{}".format(name, n)] = c.numpy()
    out["k_U0"] = uk[0].numpy()
    for n, w in enumerate(marg):
        out["marg{}".format(n)] = w.numpy()
    for name, b in bnd.items():
        out["bnd_" + name] = np.array(b)

    def T(cores, Us=None):
        return tn.Tensor([c.clone() for c in cores], Us=None if Us is None else [None if U is None else U.clone() for U in Us])

    def record(name, ref_value, truth, bound=1e-12):
        ref_value = np.asarray(ref_value, dtype=np.float64)
        err = np.abs(ref_value - truth).max() / np.abs(truth).max()
        print("{:26s} max |truth| {:.6g}  reference error {:.2e}".format(name, np.abs(truth).max(), err))
        assert err < bound, "{}: the reference is {:.2e} off the truth".format(name, err)
        out["truth_" + name], out["ref_" + name] = truth, ref_value

    a, v, k = dense(ca), dense(cv), dense(ck, uk)
    f = [dense(c) for c in cf]
    for d in (0, 1, 3):
        for o in (1, 2, 3):
            for p in (0, 1):
                Mx = np.linalg.matrix_power(stencil(a.shape[d], bnd["a"][d], bool(p)), o)
                record("partial_a_d{}_o{}_p{}".format(d, o, p),
                       tn.partial(T(ca), d, order=o, bounds=bnd["a"][d], periodic=bool(p)).numpy(), along(a, d, Mx))
    for o in (1, 2, 3):
        for p in (0, 1):
            Mx = np.linalg.matrix_power(stencil(6, bnd["k"][0], bool(p)), o)
            res = tn.partial(T(ck, uk), 0, order=o, bounds=bnd["k"][0], periodic=bool(p))
            assert res.Us[0] is not None
            record("partial_k_d0_o{}_p{}".format(o, p), res.numpy(), along(k, 0, Mx))
    record("partial_v_o1", tn.partial(T(cv), 0, bounds=bnd["v"][0]).numpy(), along(v, 0, stencil(6, bnd["v"][0])))
    record("partial_f0_default", tn.partial(T(cf[0]), 0).numpy(), along(f[0], 0, stencil(5, [0, 5])))
    grad = tn.gradient(T(ca), bounds=bnd["a"])
    for n in range(4):
        record("gradient_a_{}".format(n), grad[n].numpy(), along(a, n, stencil(a.shape[n], bnd["a"][n])))

    def lap(x, bs):
        return sum(along(x, n, np.linalg.matrix_power(stencil(x.shape[n], bs[n]), 2)) for n in range(x.ndim))

    record("laplacian_a", tn.laplacian(T(ca), bounds=bnd["a"]).numpy(), lap(a, bnd["a"]))
    record("laplacian_f0", tn.laplacian(T(cf[0]), bounds=bnd["f"]).numpy(), lap(f[0], bnd["f"]))
    record("laplacian_k", tn.laplacian(T(ck, uk), bounds=bnd["k"]).numpy(), lap(k, bnd["k"]))
    record("laplacian_v", tn.laplacian(T(cv), bounds=bnd["v"]).numpy(), lap(v, bnd["v"]))

    def dd(x, n):
        return along(x, n, stencil(5, bnd["f"][n]))

    record("divergence_f", tn.divergence([T(c) for c in cf], bounds=bnd["f"]).numpy(), dd(f[0], 0) + dd(f[1], 1) + dd(f[2], 2))
    rc = tn.curl([T(c) for c in cf], bounds=bnd["f"])
    truth_curl = [dd(f[2], 1) - dd(f[1], 2), dd(f[0], 2) - dd(f[2], 0), dd(f[1], 0) - dd(f[0], 1)]
    for n in range(3):
        record("curl_f_{}".format(n), rc[n].numpy(), truth_curl[n])

    ga = [along(a, n, stencil(a.shape[n], bnd["a"][n])) for n in range(4)]
    w_full = [(m / m.sum()).numpy() for m in marg]
    pdf = np.einsum("i,j,k,l->ijkl", *w_full)
    record("dgsm_a", tn.dgsm(T(ca), bnd["a"], [m.clone() for m in marg]).numpy(), np.array([(gn * gn * pdf).sum() for gn in ga]), 1e-5)
    w_mid = []
    for m in marg:
        mid = ((m[:-1] + m[1:]) / 2).numpy()
        w_mid.append(np.concatenate([mid / mid.sum(), [0.0]]))
    pdf = np.einsum("i,j,k,l->ijkl", *w_mid)
    M = np.array([[(ga[i] * ga[j] * pdf).sum() for j in range(4)] for i in range(4)])
    tw, tv = np.linalg.eigh(M)
    tw, tv = tw[::-1].copy(), tv[:, ::-1].copy()
    gaps = np.abs(np.diff(tw)).min() / tw[0]
    print("active_subspace eigenvalues", tw, "smallest gap / largest", gaps)
    assert gaps >= 0.1, "eigenvalues too close ({:.3g} of the largest): pick another seed".format(gaps)
    rw, rv = tn.active_subspace(T(ca), bnd["a"], [m.clone() for m in marg])
    out["truth_as_M"] = M
    record("as_w", rw.numpy(), tw, 1e-5)
    sign = np.sign((rv.numpy().astype(np.float64) * tv).sum(axis=0))
    record("as_v", rv.numpy() * sign, tv, 1e-5)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

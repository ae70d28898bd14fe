"""The cases of tests/golden/anova_f64.npz (tools/gen_anova_golden.py), shared by the host and the GPU tests of
``tntorch_amd/anova.py``, and the shapes and the fp64 reference of the ``mode_sandwich`` kernel tests.  Every golden case is a call
of the public interface on trains and masks built from the stored cores, compared with the dense brute-force ANOVA of the fixture."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_Z = None


def fixture():
    global _Z
    if _Z is None:
        with np.load(os.path.join(ROOT, "tests", "golden", "anova_f64.npz")) as z:
            _Z = {k: z[k] for k in z.files}
    return _Z


def train(name, dtype, device="cpu"):
    """The train ``name`` of the fixture (``t``, ``k``, ``mask_<m>``, ``kmask_<m>``)."""
    import tntorch_amd as tn

    z = fixture()
    N = int(z[name + "_ncores"])
    cores = [torch.from_numpy(z["{}_core{}".format(name, n)]).to(dtype).to(device) for n in range(N)]
    Us = [torch.from_numpy(z["{}_U{}".format(name, n)]).to(dtype).to(device) if "{}_U{}".format(name, n) in z else None for n in range(N)]
    return tn.Tensor(cores, Us=Us)


def marginals(dtype, device="cpu", prefix="marg"):
    z = fixture()
    N = 4 if prefix == "marg" else 2
    return [torch.from_numpy(z["{}{}".format(prefix, n)]).to(dtype).to(device) for n in range(N)]


MASKS = ("only_x0", "x0", "x0_not_x2", "weight", "one_hot", "true")


def _sobol(mask, normalize, name="t", mprefix="mask_", wprefix="marg"):
    def call(tn, dt, dev):
        return tn.sobol(train(name, dt, dev), train(mprefix + mask, dt, dev), marginals(dt, dev, wprefix), normalize=normalize)
    return call


# quantity of the fixture -> the call that returns a 0-dim tensor, a vector or a one-mode tn.Tensor
CASES = {}
for _m in MASKS:
    CASES["sobol_" + _m] = _sobol(_m, True)
    CASES["sobol_{}_raw".format(_m)] = _sobol(_m, False)
CASES["sobol_uniform_x0"] = lambda tn, dt, dev: tn.sobol(train("t", dt, dev), train("mask_x0", dt, dev))
CASES["mean_dimension"] = lambda tn, dt, dev: tn.mean_dimension(train("t", dt, dev), marginals=marginals(dt, dev))
CASES["mean_dimension_x0"] = lambda tn, dt, dev: tn.mean_dimension(train("t", dt, dev), mask=train("mask_x0", dt, dev),
                                                                   marginals=marginals(dt, dev))
CASES["dimdist"] = lambda tn, dt, dev: tn.dimension_distribution(train("t", dt, dev), marginals=marginals(dt, dev))
CASES["dimdist_o2"] = lambda tn, dt, dev: tn.dimension_distribution(train("t", dt, dev), order=2, marginals=marginals(dt, dev))
CASES["dimdist_x0"] = lambda tn, dt, dev: tn.dimension_distribution(train("t", dt, dev), mask=train("mask_x0", dt, dev),
                                                                    marginals=marginals(dt, dev))
CASES["dimdist_x0_o2"] = lambda tn, dt, dev: tn.dimension_distribution(train("t", dt, dev), mask=train("mask_x0", dt, dev), order=2,
                                                                       marginals=marginals(dt, dev))
# the Tucker input
CASES["ksobol_x0"] = _sobol("x0", True, "k", "kmask_", "kmarg")
CASES["ksobol_x0_raw"] = _sobol("x0", False, "k", "kmask_", "kmarg")
CASES["kmean_dimension"] = lambda tn, dt, dev: tn.mean_dimension(train("k", dt, dev), marginals=marginals(dt, dev, "kmarg"))


def truth(q):
    return fixture()["truth_" + q]


def value(r):
    """A result as an fp64 numpy array (a one-mode Tensor is densified)."""
    if hasattr(r, "cores"):
        r = r.torch()
    return r.detach().cpu().double().numpy()


def abs_err(r, q):
    v, t = value(r), truth(q)
    assert v.shape == t.shape, (q, v.shape, t.shape)
    return float(np.abs(v - t).max())


def rel_err(r, q):
    return abs_err(r, q) / float(np.abs(truth(q)).max())


def plus_constant(t, c):
    """``t + c`` with the constant added as block cores (rank r + 1): [A, c], [[A, 0], [0, 1]], [A; 1]."""
    import tntorch_amd as tn

    cores = []
    N = t.dim()
    for n, A in enumerate(t.cores):
        r0, I, r1 = A.shape
        B = A.new_zeros((r0 + (n > 0), I, r1 + (n < N - 1)))
        B[:r0, :, :r1] = A
        if n == 0:
            B[0, :, r1] = c
        elif n < N - 1:
            B[r0, :, r1] = 1
        else:
            B[r0, :, 0] = 1
        cores.append(B)
    return tn.Tensor(cores)


# ---------------------------------------------------------------------------------------------- mode_sandwich
# (S, R, I, C): nothing a multiple of the 16-tile, both sides of a 16 edge, the rank limit 64, I below / at / above one chunk of
# 8 slices, several chunks (130 -> 17), S > 1, and the I = 1 call that computes mu^T Z mu
SANDWICH_SHAPES = [(1, 1, 7, 1), (3, 5, 7, 6), (2, 16, 9, 17), (1, 17, 33, 15), (2, 33, 40, 20), (1, 64, 12, 64), (4, 20, 130, 31),
                   (2, 5, 1, 6), (2, 7, 8, 9)]
_SW = {}


def sandwich_inputs(shape):
    """(Z, A, w, mu) in fp64 on the CPU, seeded by the shape: Z is not symmetric, mu lies near the weighted mean of A.  Every value is
    representable in fp32, so the fp32 and the fp64 runs see the same inputs as the reference."""
    S, R, I, C = shape
    g = torch.Generator().manual_seed(1000 * S + 100 * R + 10 * I + C)
    Z = torch.randn(S, R, R, generator=g, dtype=torch.float32).double()
    A = (torch.randn(R, I, C, generator=g, dtype=torch.float32) + 0.5).double()
    w = torch.rand(I, generator=g, dtype=torch.float32).double() + 0.1
    w = (w / w.sum()).float().double()
    # near the weighted mean, not on it: with I = 1 the exact mean would leave nothing to compare
    mu = (torch.einsum("i,ric->rc", w, A) + 0.1 * torch.randn(R, C, generator=g, dtype=torch.float64)).float().double()
    return Z, A, w, mu


def sandwich_reference(shape, given):
    """The fp64 einsum on the CPU, computed once per (shape, w / mu given or NULL)."""
    key = (shape, given)
    if key not in _SW:
        Z, A, w, mu = sandwich_inputs(shape)
        Ac = A - mu[:, None, :] if given else A
        ww = w if given else torch.ones_like(w)
        _SW[key] = torch.einsum("i,aic,sab,bid->scd", ww, Ac, Z, Ac)
    return _SW[key]

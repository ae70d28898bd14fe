"""The cases of tests/golden/moments_f32.npz (tools/gen_moments_golden.py) and their bounds, shared by the host and the GPU tests
of the moment family.  Every case is a call of the public interface on trains built from the stored cores; its value is compared
with the dense fp64 truth of the fixture."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_Z = None


def fixture():
    global _Z
    if _Z is None:
        with np.load(os.path.join(ROOT, "tests", "golden", "moments_f32.npz")) as z:
            _Z = {k: z[k] for k in z.files}
    return _Z


def train(name, dtype, device="cpu"):
    import tntorch_amd as tn

    z = fixture()
    return tn.Tensor([torch.from_numpy(z["{}_core{}".format(name, n)]).to(dtype).to(device) for n in range(int(z[name + "_ncores"]))])


def marginals(dtype, device="cpu"):
    z = fixture()
    return [torch.from_numpy(z["marg{}".format(n)]).to(dtype).to(device) for n in range(4)]


def _hs(names, **kw):
    def call(tn, dt, dev):
        return tn.hadamard_sum([train(n, dt, dev) for n in names], **kw)
    return call


def _raw(name, k, marg=False, **kw):
    def call(tn, dt, dev):
        return tn.raw_moment(train(name, dt, dev), k, marginals=marginals(dt, dev) if marg else None, **kw)
    return call


# quantity of the fixture -> the call whose arithmetic is exact (no rounding step): 1e-5 in fp32, 1e-12 in fp64
EXACT = {
    "hsum_exact_M1": _hs("a", algorithm="exact"),
    "hsum_exact_M2": _hs("ab", algorithm="exact"),
    "hsum_exact_M3": _hs("aba", algorithm="exact"),
    "hsum_exact_M4": _hs("abab", algorithm="exact"),
    "v_hsum_exact_M3": _hs("vvv", algorithm="exact"),
    "var": lambda tn, dt, dev: tn.var(train("a", dt, dev)),
    "varm": lambda tn, dt, dev: tn.var(train("a", dt, dev), marginals=marginals(dt, dev)),
    "std": lambda tn, dt, dev: tn.std(train("a", dt, dev)),
}
for _k in range(1, 5):
    EXACT["raw_k{}".format(_k)] = _raw("a", _k, algorithm="exact")
    EXACT["rawm_k{}".format(_k)] = _raw("a", _k, marg=True, algorithm="exact")

# quantity -> the call with the arguments the reference's value was recorded with (approximate algorithms)
APPROX = {
    "hsum_eig_M3": _hs("aba", algorithm="eig", eps=1e-6),
    "hsum_svd_M3": _hs("aba", algorithm="svd", eps=1e-6),
    "norm_k3": lambda tn, dt, dev: tn.normalized_moment(train("a", dt, dev), 3),
    "norm_k4": lambda tn, dt, dev: tn.normalized_moment(train("a", dt, dev), 4),
    "m_raw_k3": _raw("m", 3),
}
for _k in range(1, 5):
    APPROX["raw_k{}".format(_k)] = _raw("a", _k)
    APPROX["rawm_k{}".format(_k)] = _raw("a", _k, marg=True)

# fp64, "eig" at eps = 1e-12: the product ranks of the fixture trains are at most 3 * 2 * 3, so the roundings only drop
# numerically null directions; 1e-9 relative to the truth
TIGHT = {
    "hsum_eig_M3": _hs("aba", algorithm="eig", eps=1e-12),
    "norm_k3": lambda tn, dt, dev: tn.normalized_moment(train("a", dt, dev), 3),
    "norm_k4": lambda tn, dt, dev: tn.normalized_moment(train("a", dt, dev), 4),
    "m_raw_k3": _raw("m", 3, eps=1e-12),
}
for _k in range(1, 5):
    TIGHT["raw_k{}".format(_k)] = _raw("a", _k, eps=1e-12)
    TIGHT["rawm_k{}".format(_k)] = _raw("a", _k, marg=True, eps=1e-12)


def truth(q):
    return float(fixture()["truth_" + q])


def approx_bound(q):
    """max(4 x the reference's own recorded error, 1e-5 |truth|): the floor is the project's fp32 parity bound, the factor
    allows for a different but equally valid eigensolver and rank decision."""
    z = fixture()
    return max(4.0 * abs(float(z["ref_" + q]) - truth(q)), 1e-5 * abs(truth(q)))


def check_exact(q, value, dtype):
    err = abs(float(value) - truth(q)) / abs(truth(q))
    print(q, dtype, "value", float(value), "truth", truth(q), "rel. error", err)
    assert err < (1e-5 if dtype == torch.float32 else 1e-12), (q, err)


def check_approx(q, value):
    err = abs(float(value) - truth(q))
    print(q, "value", float(value), "truth", truth(q), "error", err, "bound", approx_bound(q))
    assert err <= approx_bound(q), (q, err, approx_bound(q))


def check_tight(q, value):
    err = abs(float(value) - truth(q)) / abs(truth(q))
    print(q, "value", float(value), "truth", truth(q), "rel. error", err)
    assert err < 1e-9, (q, err)

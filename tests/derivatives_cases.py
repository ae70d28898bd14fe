"""The cases of tests/golden/derivatives_f64.npz (tools/gen_derivatives_golden.py), shared by the host and the GPU tests of
``tntorch_amd/derivatives.py``.  Every case is a call of the public interface on trains built from the stored cores; tensor-valued
results are densified and compared with the dense fp64 truth of the fixture."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_Z = None


def fixture():
    global _Z
    if _Z is None:
        with np.load(os.path.join(ROOT, "tests", "golden", "derivatives_f64.npz")) as z:
            _Z = {k: z[k] for k in z.files}
    return _Z


def train(name, dtype, device="cpu"):
    import tntorch_amd as tn

    z = fixture()
    N = int(z[name + "_ncores"])
    cores = [torch.from_numpy(z["{}_core{}".format(name, n)]).to(dtype).to(device) for n in range(N)]
    Us = [torch.from_numpy(z["{}_U{}".format(name, n)]).to(dtype).to(device) if "{}_U{}".format(name, n) in z else None for n in range(N)]
    return tn.Tensor(cores, Us=Us)


def bounds(name):
    return [[float(b0), float(b1)] for b0, b1 in fixture()["bnd_" + name]]


def marginals(dtype, device="cpu"):
    z = fixture()
    return [torch.from_numpy(z["marg{}".format(n)]).to(dtype).to(device) for n in range(4)]


def _partial(name, d, o, p):
    def call(tn, dt, dev):
        return tn.partial(train(name, dt, dev), d, order=o, bounds=bounds(name)[d], periodic=bool(p))
    return call


def _field(dt, dev):
    return [train("f{}".format(n), dt, dev) for n in range(3)]


# quantity of the fixture -> the call that returns a tn.Tensor
TENSOR = {
    "partial_v_o1": lambda tn, dt, dev: tn.partial(train("v", dt, dev), 0, bounds=bounds("v")[0]),
    "partial_f0_default": lambda tn, dt, dev: tn.partial(train("f0", dt, dev), 0),
    "laplacian_a": lambda tn, dt, dev: tn.laplacian(train("a", dt, dev), bounds=bounds("a")),
    "laplacian_f0": lambda tn, dt, dev: tn.laplacian(train("f0", dt, dev), bounds=bounds("f")),
    "laplacian_k": lambda tn, dt, dev: tn.laplacian(train("k", dt, dev), bounds=bounds("k")),
    "laplacian_v": lambda tn, dt, dev: tn.laplacian(train("v", dt, dev), bounds=bounds("v")),
    "divergence_f": lambda tn, dt, dev: tn.divergence(_field(dt, dev), bounds=bounds("f")),
}
for _o in (1, 2, 3):
    for _p in (0, 1):
        for _d in (0, 1, 3):
            TENSOR["partial_a_d{}_o{}_p{}".format(_d, _o, _p)] = _partial("a", _d, _o, _p)
        TENSOR["partial_k_d0_o{}_p{}".format(_o, _p)] = _partial("k", 0, _o, _p)
for _n in range(4):
    TENSOR["gradient_a_{}".format(_n)] = lambda tn, dt, dev, n=_n: tn.gradient(train("a", dt, dev), bounds=bounds("a"))[n]
for _n in range(3):
    TENSOR["curl_f_{}".format(_n)] = lambda tn, dt, dev, n=_n: tn.curl(_field(dt, dev), bounds=bounds("f"))[n]


def dgsm(tn, dt, dev):
    return tn.dgsm(train("a", dt, dev), bounds("a"), marginals(dt, dev))


def as_matrix(tn, dt, dev):
    from tntorch_amd import derivatives

    return derivatives._as_matrix(train("a", dt, dev), bounds("a"), marginals(dt, dev))


def active_subspace(tn, dt, dev):
    return tn.active_subspace(train("a", dt, dev), bounds("a"), marginals(dt, dev))


def truth(q):
    return fixture()["truth_" + q]


def ref(q):
    return fixture()["ref_" + q]


def rel_err(value, q, against=None):
    """max |value - truth_q| relative to the largest entry of truth_q."""
    t = truth(q) if against is None else against
    v = value.detach().cpu().double().numpy() if isinstance(value, torch.Tensor) else np.asarray(value, dtype=np.float64)
    assert v.shape == t.shape, (q, v.shape, t.shape)
    return float(np.abs(v - t).max() / np.abs(truth(q)).max())


def check_tensor(q, t, dtype):
    """A tensor-valued result, densified: 1e-12 (fp64) / 5e-6 (fp32) of the largest entry of the truth."""
    err = rel_err(t.torch(), q)
    print(q, dtype, "rel. error", err)
    assert err < (5e-6 if dtype == torch.float32 else 1e-12), (q, err)


def align_signs(v, q="as_v"):
    """Eigenvectors are compared up to sign: flip each column of ``v`` to the orientation of the truth."""
    v = v.detach().cpu().double().numpy()
    return v * np.sign((v * truth(q)).sum(axis=0))

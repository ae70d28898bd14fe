"""The cases of tests/golden/arraytools_f64.npz (tools/gen_arraytools_golden.py) and the test-side truths of the array tools
(``tn.cat``, ``tn.flip``, ``tn.ttm``, ``tn.cumsum``, ``tn.pad``, ...), shared by the generator, the host tests and the GPU tests.

A case is a function of a module ``tn`` (the reference when the fixture is recorded, this package in the tests), the input trains
``T`` and the auxiliary factors ``A``; its result -- a tensor train, a list of them, or a torch matrix -- is compared densified."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "arraytools_f64.npz")
U32, U64 = 2.0 ** -24, 2.0 ** -53
TENSORS = ("p", "q", "k", "b", "s", "v")
# the auxiliary factors: name -> shape (drawn by the generator, stored as aux_<name>)
AUX = {"A1": (6, 4), "A0t": (3, 2), "A2t": (5, 4), "w1": (4,), "Ak": (3, 6), "wk": (6,), "B0": (2, 3), "B1": (3, 4)}
BASES = ("dct", "identity", "legendre", "chebyshev", "hermite")
BASIS_SHAPES = ((5, 3), (4, 4))

CASES = {
    # cat: on each mode, of three tensors, with Tucker factors on and off `dim`, mixed, and with open boundary ranks
    "cat_pp_0": lambda tn, T, A: tn.cat([T["p"], T["p"]], dim=0),
    "cat_pq_1": lambda tn, T, A: tn.cat([T["p"], T["q"]], dim=1),
    "cat_pp_2": lambda tn, T, A: tn.cat(T["p"], T["p"], dim=2),
    "cat_pqp_1": lambda tn, T, A: tn.cat([T["p"], T["q"], T["p"]], dim=1),
    "cat_kk_0": lambda tn, T, A: tn.cat([T["k"], T["k"]], dim=0),
    "cat_kk_1": lambda tn, T, A: tn.cat([T["k"], T["k"]], dim=1),
    "cat_kd_0": lambda tn, T, A: tn.cat([T["k"], T["k"].decompress_tucker_factors()], dim=0),
    "cat_vv_0": lambda tn, T, A: tn.cat([T["v"], T["v"]], dim=0),
    "transpose_p": lambda tn, T, A: tn.transpose(T["p"]),
    "transpose_k": lambda tn, T, A: tn.transpose(T["k"]),
    "transpose_b": lambda tn, T, A: tn.transpose(T["b"]),
    "flip_p_1": lambda tn, T, A: tn.flip(T["p"], 1),
    "flip_p_02": lambda tn, T, A: tn.flip(T["p"], [0, 2]),
    "flip_k_0": lambda tn, T, A: tn.flip(T["k"], 0),
    "flip_b_1": lambda tn, T, A: tn.flip(T["b"], 1),
    # ttm: a matrix on one mode, two modes at once with transpose=True, a vector, a Tucker mode, dim=None
    "ttm_p_1": lambda tn, T, A: tn.ttm(T["p"], A["A1"], dim=1),
    "ttm_p_02t": lambda tn, T, A: tn.ttm(T["p"], [A["A0t"], A["A2t"]], dim=[0, 2], transpose=True),
    "ttm_p_vec1": lambda tn, T, A: tn.ttm(T["p"], A["w1"], dim=1),
    "ttm_p_default": lambda tn, T, A: tn.ttm(T["p"], [A["B0"], A["B1"]]),
    "ttm_k_0": lambda tn, T, A: tn.ttm(T["k"], A["Ak"], dim=0),
    "ttm_k_vec0": lambda tn, T, A: tn.ttm(T["k"], A["wk"], dim=0),
    "ttm_p_neg": lambda tn, T, A: tn.ttm(T["p"], A["A2t"].t(), dim=-1),
    "cumsum_p_1": lambda tn, T, A: tn.cumsum(T["p"], 1),
    "cumsum_p_all": lambda tn, T, A: tn.cumsum(T["p"]),
    "cumsum_k_0": lambda tn, T, A: tn.cumsum(T["k"], 0),
    "cumsum_k_all": lambda tn, T, A: tn.cumsum(T["k"]),
    "cumsum_b_all": lambda tn, T, A: tn.cumsum(T["b"]),
    "pad_p": lambda tn, T, A: tn.pad(T["p"], [4, 6, 5]),
    "pad_p_1": lambda tn, T, A: tn.pad(T["p"], 7, dim=1),
    "pad_k_0": lambda tn, T, A: tn.pad(T["k"], 8, dim=0),
    "squeeze_s": lambda tn, T, A: tn.squeeze(T["s"]),
    "squeeze_s_2": lambda tn, T, A: tn.squeeze(T["s"], 2),
    "unsqueeze_p": lambda tn, T, A: tn.unsqueeze(T["p"], [0, 2]),
    "unsqueeze_v": lambda tn, T, A: tn.unsqueeze(T["v"], 1),
    "unbind_p_1": lambda tn, T, A: tn.unbind(T["p"], 1),
    "unbind_k_0": lambda tn, T, A: tn.unbind(T["k"], 0),
}

_Z = None


def fixture():
    global _Z
    if _Z is None:
        with np.load(GOLDEN) as z:
            _Z = {k: z[k] for k in z.files}
    return _Z


def cases():
    return sorted(CASES)


def dense_cores(cores, Us):
    """fp64 densification of cores [r, I, r'] and factors: an array [r_0, I_1, .., I_N, r_N] without the boundary ranks of 1."""
    out = None
    shape = []
    for c, U in zip(cores, Us):
        c = c.detach().cpu().double().numpy()
        if U is not None:
            c = np.einsum("aib,ji->ajb", c, U.detach().cpu().double().numpy())
        shape.append(c.shape[1])
        out = c.reshape(c.shape[0], -1) if out is None else (out @ c.reshape(c.shape[0], -1))
        first = out.shape[0] if len(shape) == 1 else first
        out = out.reshape(-1, c.shape[2])
    full = [first] + shape + [out.shape[1]]
    out = out.reshape(full)
    if full[-1] == 1:
        out = out[..., 0]
    if full[0] == 1:
        out = out[0]
    return out


def dense(x):
    """What a case returns -- a tensor train of either module, a list of them, a torch tensor -- as an fp64 array."""
    if isinstance(x, (list, tuple)):
        return np.stack([dense(y) for y in x])
    if hasattr(x, "cores"):
        return dense_cores(x.cores, x.Us)
    return x.detach().cpu().double().numpy()


def train(name, dtype, device="cpu", module=None):
    if module is None:
        import tntorch_amd as module
    z = fixture()
    N = int(z[name + "_ncores"])
    cores = [torch.from_numpy(z["{}_core{}".format(name, n)]).to(dtype).to(device) for n in range(N)]
    Us = [torch.from_numpy(z["{}_U{}".format(name, n)]).to(dtype).to(device) if "{}_U{}".format(name, n) in z else None for n in range(N)]
    return module.Tensor(cores, Us=Us)


def inputs(dtype, device="cpu"):
    """(T, A): the input trains and the auxiliary factors of the fixture in ``dtype`` on ``device``."""
    z = fixture()
    T = {name: train(name, dtype, device) for name in TENSORS}
    A = {name: torch.from_numpy(z["aux_" + name]).to(dtype).to(device) for name in AUX}
    return T, A


def snapshot(T, A):
    """Bit copies of every core, factor and auxiliary tensor: for 'inputs are unchanged' checks."""
    out = {}
    for name, t in T.items():
        for n, (c, U) in enumerate(zip(t.cores, t.Us)):
            out[(name, n, "core")] = c.detach().cpu().clone()
            if U is not None:
                out[(name, n, "U")] = U.detach().cpu().clone()
    for name, a in A.items():
        out[(name, "aux")] = a.detach().cpu().clone()
    return out


def unchanged(T, A, snap):
    now = snapshot(T, A)
    return set(now) == set(snap) and all(torch.equal(now[k], snap[k]) for k in snap)


def truth(case):
    return fixture()["out_" + case]


def rel_err(value, reference):
    """Relative Frobenius error of a dense array."""
    value, reference = np.asarray(value, dtype=np.float64), np.asarray(reference, dtype=np.float64)
    assert value.shape == reference.shape, (value.shape, reference.shape)
    return float(np.linalg.norm(value - reference) / np.linalg.norm(reference))


def tol(dtype):
    """Relative Frobenius tolerances of test_moments_host.py."""
    return 1e-12 if dtype == torch.float64 else 1e-5


def rand_train(shape, rank, g, dtype, tucker=(), device="cpu"):
    """A random train of ``shape`` with TT ranks ``rank``; the modes in ``tucker`` get a factor [I, max(1, I - 1)]."""
    import tntorch_amd as tn

    rs = [1] + [rank] * (len(shape) - 1) + [1]
    cores, Us = [], []
    for n, I in enumerate(shape):
        S = max(1, I - 1) if n in tucker else I
        cores.append(torch.rand(rs[n], S, rs[n + 1], generator=g, dtype=torch.float64).to(dtype).to(device))
        Us.append(torch.rand(I, S, generator=g, dtype=torch.float64).to(dtype).to(device) if n in tucker else None)
    return tn.Tensor(cores, Us=Us)


# ---------------------------------------------------------------------------------------------- dense truths the reference cannot give
def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _pad7(d, shape):
    widths = []
    for have, want in reversed(list(zip(d.shape, shape))):
        widths += [0, want - have]
    return torch.nn.functional.pad(_t(d), widths, value=7.0).numpy()


# name -> function(tn, T, A) -> (result of the package, truth from the fp64 densification of the same (rounded) inputs)
DENSE_TRUTHS = {
    "cat_pq_1": lambda tn, T, A: (tn.cat([T["p"], T["q"], T["p"]], dim=1), torch.cat([_t(dense(T["p"])), _t(dense(T["q"])), _t(dense(T["p"]))], 1).numpy()),
    "cat_kk_0": lambda tn, T, A: (tn.cat([T["k"], T["k"]], dim=0), torch.cat([_t(dense(T["k"]))] * 2, 0).numpy()),
    "cat_kk_-1": lambda tn, T, A: (tn.cat(T["k"], T["k"], dim=-1), torch.cat([_t(dense(T["k"]))] * 2, 1).numpy()),
    "flip_p_02": lambda tn, T, A: (tn.flip(T["p"], [0, 2]), torch.flip(_t(dense(T["p"])), [0, 2]).numpy()),
    "flip_k_0": lambda tn, T, A: (tn.flip(T["k"], 0), torch.flip(_t(dense(T["k"])), [0]).numpy()),
    "cumsum_p_all": lambda tn, T, A: (tn.cumsum(T["p"]), _t(dense(T["p"])).cumsum(0).cumsum(1).cumsum(2).numpy()),
    "cumsum_p_-1": lambda tn, T, A: (tn.cumsum(T["p"], -1), _t(dense(T["p"])).cumsum(2).numpy()),
    "cumsum_k_all": lambda tn, T, A: (tn.cumsum(T["k"]), _t(dense(T["k"])).cumsum(0).cumsum(1).numpy()),
    "pad7_p": lambda tn, T, A: (tn.pad(T["p"], [4, 6, 5], fill_value=7), _pad7(dense(T["p"]), [4, 6, 5])),
    "pad7_p_1": lambda tn, T, A: (tn.pad(T["p"], 6, dim=1, fill_value=7), _pad7(dense(T["p"]), [3, 6, 5])),
    "pad7_k": lambda tn, T, A: (tn.pad(T["k"], [8, 7], fill_value=7), _pad7(dense(T["k"]), [8, 7])),
    "pad7_v": lambda tn, T, A: (tn.pad(T["v"], 6, fill_value=7), _pad7(dense(T["v"]), [6])),
    "transpose_p": lambda tn, T, A: (tn.transpose(T["p"]), dense(T["p"]).transpose(2, 1, 0)),
    "ttm_p_1": lambda tn, T, A: (tn.ttm(T["p"], A["A1"], dim=1), np.einsum("iak,ja->ijk", dense(T["p"]), dense(A["A1"]))),
    "ttm_p_02t": lambda tn, T, A: (tn.ttm(T["p"], [A["A0t"], A["A2t"]], dim=[0, 2], transpose=True),
                                   np.einsum("iak,ix,ky->xay", dense(T["p"]), dense(A["A0t"]), dense(A["A2t"]))),
    "ttm_k_0": lambda tn, T, A: (tn.ttm(T["k"], A["Ak"], dim=0), np.einsum("ik,ji->jk", dense(T["k"]), dense(A["Ak"]))),
    "marginal_p_1": lambda tn, T, A: (tn.squeeze(tn.ttm(T["p"], A["w1"], dim=1)), np.einsum("iak,a->ik", dense(T["p"]), dense(A["w1"]))),
    "marginal_k_0": lambda tn, T, A: (tn.squeeze(tn.ttm(T["k"], A["wk"], dim=0)), np.einsum("ik,i->k", dense(T["k"]), dense(A["wk"]))),
    "unbind_p_2": lambda tn, T, A: (tn.unbind(T["p"], 2), dense(T["p"]).transpose(2, 0, 1)),
    "unsqueeze_squeeze": lambda tn, T, A: (tn.squeeze(tn.unsqueeze(T["p"], [1, 4])), dense(T["p"])),
}


def reduce_cat(tn, dtype, device="cpu", rmax=12):
    """(result, truth): ``tn.reduce([t1 .. t5], tn.cat, dim=1, rmax=rmax)`` of five random 3 x (2..4) x 4 trains of rank 2 (the
    exact ranks are at most 3 and 4: nothing is truncated) and the dense concatenation."""
    g = torch.Generator().manual_seed(5)
    ts = [rand_train([3, 2 + n % 3, 4], 2, g, dtype, device=device) for n in range(5)]
    return tn.reduce(ts, tn.cat, dim=1, rmax=rmax), np.concatenate([dense(t) for t in ts], axis=1)


# ---------------------------------------------------------------------------------------------- the core-level (kernel) cases
KERNEL_SHAPES = [(1, 1, 1), (1, 2, 1), (3, 5, 7), (1, 5, 3), (3, 5, 1), (2, 3, 17), (1, 64, 64), (2, 65, 3), (2, 130, 65),
                 (3, 257, 5), (1, 1000, 1), (1, 4100, 2), (64, 64, 64)]


def kernel_input(shape, dtype, seed=0):
    """(X, w): a random core [R, I, C] and weights [I], drawn in fp64 and rounded to ``dtype`` (CPU tensors)."""
    g = torch.Generator().manual_seed(seed + 7 * shape[0] + 3 * shape[1] + shape[2])
    return (torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype), torch.randn(shape[1], generator=g, dtype=torch.float64).to(dtype))


def scan_truth(X):
    """(truth, A): the fp64 running sum of the (rounded) input on the CPU and that of its absolute values."""
    Xd = X.detach().cpu().double()
    return torch.cumsum(Xd, 1), torch.cumsum(Xd.abs(), 1)


def reduce_truth(X, w, scale):
    """(truth, A): scale * sum_i w[i] X[:, i, :] in fp64 on the CPU and |scale| sum |w| |X|; ``w`` None: ones."""
    Xd = X.detach().cpu().double()
    wd = torch.ones(Xd.shape[1], dtype=torch.float64) if w is None else w.detach().cpu().double()
    return scale * torch.einsum("i,ric->rc", wd, Xd), abs(scale) * torch.einsum("i,ric->rc", wd.abs(), Xd.abs())


def kernel_bound(kind, I, dtype, truth, A):
    """Entry-wise, derived: fp64 accumulation in any order errs by at most (I - 1) 2^-53 A to first order (+ the product and the
    scaling for the reduction), taken with a factor 2 to spare -- I 2^-52 A for the scan, (I + 2) 2^-52 A for the reduction; fp32
    results add the one rounding at the store, 2^-23 |truth| (twice the half-ulp: the stored value rounds the erring sum)."""
    b = (I if kind == "scan" else I + 2) * 2.0 ** -52 * A
    if dtype == torch.float32:
        b = b + 2.0 ** -23 * truth.abs()
    return b

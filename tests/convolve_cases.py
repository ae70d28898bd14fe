"""The cases of tests/golden/convolve_f64.npz (tools/gen_convolve_golden.py) and the test-side truth of ``tn.convolve``, shared by
the host and the GPU tests: np.convolve's windows, a dense fp64 convolution, the fp64 host mirror and the derived fp32 bound."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("full", "same", "valid")
U32, U64 = 2.0 ** -24, 2.0 ** -53
_Z = None


def fixture():
    global _Z
    if _Z is None:
        with np.load(os.path.join(ROOT, "tests", "golden", "convolve_f64.npz")) as z:
            _Z = {k: z[k] for k in z.files}
    return _Z


def cases():
    """Every recorded case "<a><b>_<mode>", sorted."""
    return sorted(k[len("truth_"):] for k in fixture() if k.startswith("truth_"))


def reference_cases():
    """The cases where the reference is defined (its result and its error against the truth are recorded)."""
    return [c for c in cases() if "referr_" + c in fixture()]


def split(case):
    pair, mode = case.split("_")
    return pair[0], pair[1], mode


def train(name, dtype, device="cpu"):
    import tntorch_amd as tn

    z = fixture()
    N = int(z[name + "_ncores"])
    cores = [torch.from_numpy(z["{}_core{}".format(name, n)]).to(dtype).to(device) for n in range(N)]
    Us = [torch.from_numpy(z["{}_U{}".format(name, n)]).to(dtype).to(device) if "{}_U{}".format(name, n) in z else None for n in range(N)]
    return tn.Tensor(cores, Us=Us)


def operands(case, dtype, device="cpu"):
    a, b, mode = split(case)
    return train(a, dtype, device), train(b, dtype, device), mode


def truth(case):
    return fixture()["truth_" + case]


def referr(case):
    return float(fixture()["referr_" + case])


def window(I, J, mode):
    """(lo, K) of np.convolve(x, y, mode) inside the full result, len(x) = I, len(y) = J."""
    k, m = min(I, J), max(I, J)
    return {"full": (0, I + J - 1), "same": ((k - 1) // 2, m), "valid": (k - 1, m - k + 1)}[mode]


def dense_convolve(x, y, mode="full"):
    """N-d convolution of two dense fp64 arrays, cropped per mode with ``window``: one shifted multiply-add per entry of y."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    full = np.zeros([I + J - 1 for I, J in zip(x.shape, y.shape)])
    for idx in np.ndindex(*y.shape):
        full[tuple(slice(j, j + I) for j, I in zip(idx, x.shape))] += y[idx] * x
    wins = [window(I, J, mode) for I, J in zip(x.shape, y.shape)]
    return full[tuple(slice(lo, lo + K) for lo, K in wins)]


def cores64(t):
    """fp64 CPU cores [r, I, r'] of a tn.Tensor with its Tucker factors contracted in."""
    out = []
    for c, U in zip(t.cores, t.Us):
        c = c.detach().cpu().double()
        if U is not None:
            c = torch.einsum("aib,ji->ajb", c, U.detach().cpu().double())
        out.append(c)
    return out


def dense64(t):
    """A tn.Tensor (or a list of cores) densified in fp64 on the CPU, whatever its dtype and device."""
    cores = cores64(t) if hasattr(t, "cores") else [c.detach().cpu().double() for c in t]
    out = torch.ones(1, 1, dtype=torch.float64)
    for c in cores:
        out = (out @ c.reshape(c.shape[0], -1)).reshape(-1, c.shape[2])
    return out.reshape([c.shape[1] for c in cores]).numpy()


def mirror64(a, c, lo, K):
    """The fp64 host mirror of ttr_core_convolve on the values of a and c (whatever their dtype and device)."""
    from tntorch_amd import _hostops

    return _hostops.core_convolve(a.detach().cpu().double(), c.detach().cpu().double(), lo, K)


def mirror_train(t1, t2, mode, absolute=False):
    """The exact convolution train from the fp64 mirror (``absolute``: of the entry-wise absolute values of the cores)."""
    a, b = cores64(t1), cores64(t2)
    if absolute:
        a, b = [x.abs() for x in a], [x.abs() for x in b]
    return [mirror64(x, y, *window(x.shape[1], y.shape[1], mode)) for x, y in zip(a, b)]


def rel_err(value, reference):
    """Relative Frobenius error of a dense array."""
    value, reference = np.asarray(value, dtype=np.float64), np.asarray(reference, dtype=np.float64)
    assert value.shape == reference.shape, (value.shape, reference.shape)
    return float(np.linalg.norm(value - reference) / np.linalg.norm(reference))


def fp32_exact_bound(t1, t2, mode, reference):
    """The fp32 bound of the exact path relative to ||reference||: every core entry is a sum of n <= n_max = max_n min(I_n, J_n)
    products, accumulated with at most n roundings plus the one at the store, (n + 2) u |a| * |c| per entry with spare; to first
    order the errors of the N cores add up in the train of the absolute values:  N (n_max + 2) 2^-24 ||absconv train||."""
    n_max = max(min(I, J) for I, J in zip(t1.shape, t2.shape))
    absnorm = float(np.linalg.norm(dense64(mirror_train(t1, t2, mode, absolute=True))))
    return t1.dim() * (n_max + 2) * U32 * absnorm / float(np.linalg.norm(reference))


# ---------------------------------------------------------------------------------------------- the core-level (kernel) cases
TILE_C = 64                      # output columns per workgroup
TILE_K = (16, 32, 64)            # values of k per workgroup: one element per store / 16-byte stores in fp64 / in fp32
# (R1, I, R2), (S1, J, S2)
KERNEL_SHAPES = [
    ((1, 1, 1), (1, 1, 1)),                                  # all ones
    ((2, 1, 3), (3, 5, 2)), ((3, 5, 2), (2, 1, 3)),          # I = 1, J = 1
    ((3, 5, 7), (2, 4, 3)), ((2, 4, 3), (3, 5, 7)),          # I > J, I < J
    ((2, 5, 2), (2, 5, 2)), ((2, 4, 2), (2, 4, 2)),          # I = J, odd and even
    ((1, 5, 3), (1, 4, 2)), ((3, 5, 1), (2, 4, 1)),          # a first and a last core
    ((2, 3, 5), (3, 2, 7)),                                  # 35 columns: no multiple of 4 nor of 64
    # 63 / 64 / 65 columns (one tile less one, one tile, two tiles) with K = I + J - 1 around the k tiles of their path:
    # 63 and 65 columns store single elements (k tile 16), 64 columns 16 bytes (k tile 32 in fp64, 64 in fp32)
    ((1, 9, 9), (1, 7, 7)), ((1, 9, 9), (1, 8, 7)), ((1, 9, 9), (1, 9, 7)),            # 63 columns, K = 15, 16, 17
    ((1, 9, 13), (1, 7, 5)), ((1, 9, 13), (1, 8, 5)), ((1, 9, 13), (1, 9, 5)),         # 65 columns, K = 15, 16, 17
    ((1, 16, 8), (1, 16, 8)), ((1, 17, 8), (1, 16, 8)), ((1, 17, 8), (1, 17, 8)),      # 64 columns, K = 31, 32, 33
    ((1, 32, 8), (1, 32, 8)), ((1, 33, 8), (1, 32, 8)), ((1, 33, 8), (1, 33, 8)),      # 64 columns, K = 63, 64, 65; 32 / 33 terms
    ((1, 3, 17), (1, 2, 4)),                                 # 68 columns: 16-byte stores into a partial second tile
    ((1, 3, 11), (1, 2, 6)),                                 # 66 columns: 16-byte stores in fp64 only
    # the sum over the shorter mode on both sides of the staged limit of 32 terms, either argument the shorter one
    ((2, 31, 2), (2, 40, 2)), ((2, 32, 2), (2, 40, 2)), ((2, 33, 2), (2, 40, 2)), ((2, 40, 2), (2, 33, 2)),
    ((1, 70, 2), (2, 65, 1)),                                # 65 terms: three chunks
    ((16, 65, 16), (4, 9, 4)),                               # 64 rows x 64 columns x K = 73: many workgroups, two k tiles
]


def kernel_windows(I, J):
    """full, same, valid and, where the full result has room for it, the interior window (lo, K) = (2, 3)."""
    w = [window(I, J, m) for m in MODES]
    if I + J - 1 >= 5:
        w.append((2, 3))
    return w


def kernel_inputs(sa, sc, dtype, seed=0):
    """Random cores of the two shapes, drawn in fp64 and rounded to ``dtype`` (CPU tensors)."""
    g = torch.Generator().manual_seed(seed + 7 * sum(sa) + sum(sc))
    return (torch.randn(*sa, generator=g, dtype=torch.float64).to(dtype), torch.randn(*sc, generator=g, dtype=torch.float64).to(dtype))


def kernel_bound(I, J, dtype, absconv):
    """Derived, per entry: a sum of n <= min(I, J) products accumulates at most n rounding errors, plus the one at the store."""
    return (min(I, J) + 2) * (U32 if dtype == torch.float32 else U64) * absconv

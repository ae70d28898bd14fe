"""What the tests of ``tn.tt_eigsh``, of its ops (``ritz_gram``, ``ritz_update``) and of the kernels behind them share.  The
matrices are those of ``solve_cases`` and three more; every truth is ``torch.linalg.eigh`` of the dense fp64 matrix and
independent of the package.  At import every matrix is checked for exact symmetry and for a relative gap
``(l2 - l1) / (ln - l1) >= 0.05`` at both ends of its spectrum (the convergence rate of the local solver depends on it)."""
import functools
import math

import torch

import solve_cases as sc

DTYPES = sc.DTYPES
unit, dense_matrix, dense_train, dense = sc.unit, sc.dense_matrix, sc.dense_train, sc.dense
WHICH = ["SA", "LA"]


def eps(dt):
    return float(torch.finfo(dt).eps)


# ------------------------------------------------------------------ matrices: name -> (fp64 cores, dims)
def _build():
    out = {name: (build(dims), dims) for name, (build, dims) in sc.MATRICES.items()}
    out["indef"] = (sc.laplace_cores([4, 3, 5], shift=-1.5), [4, 3, 5])      # spectrum [-1.191, 1.191]
    out["one"] = (sc.laplace_cores([7]), [7])
    out["two"] = (sc.shifted_cores([6, 5]), [6, 5])
    return out


def lap(n):
    """The 1-D Laplacian tridiag(-1, 2, -1) the laplace matrices are made of (fp64)."""
    return sc._lap(n)


MATRICES = _build()
FULL_RANKS = dict(sc.FULL_RANKS, indef=[4, 5], one=[], two=[5])
RANK_ONE = ["kron", "laplace", "laplace4", "indef"]      # their extreme eigenvectors are rank 1 (test_eigs_host checks it by SVD)
RANK_TWO = ["shifted", "two"]                            # variational cases
MIN_GAP = 0.05


def _gaps(w):
    spread = float(w[-1] - w[0])
    return float(w[1] - w[0]) / spread, float(w[-1] - w[-2]) / spread


for _name, (_cores, _dims) in MATRICES.items():
    _D = dense_matrix(_cores)
    assert torch.equal(_D, _D.t()), _name
    _lo, _hi = _gaps(torch.linalg.eigvalsh(_D))
    assert _lo >= MIN_GAP and _hi >= MIN_GAP, "{} {}: relative gaps {:.3f} (lower end) {:.3f} (upper end)".format(_name, _dims, _lo, _hi)

# ------------------------------------------------------------------ tolerances and the measured bounds
TOL = {torch.float32: None, torch.float64: 1e-9}


def tol_of(dt):
    return math.sqrt(eps(dt)) if TOL[dt] is None else TOL[dt]


# The worst case of the host mirror over the full-rank cases (every matrix, SA and LA) and the rank-1 cases (RANK_ONE, SA and LA),
# starts drawn after torch.manual_seed(s) for s = 0 .. 4, tol as above, local_iters = 50 (tools/eigs_bench.py --bounds prints
# them): the relative error of the value against the dense eigenvalue of the cast matrix and the dense residual
# ||D x - value x|| / ||D x||.  The bound of the host AND the device tests is 4 x the worst case.
MEASURED_VALUE_ERROR = {torch.float32: 5.60e-7, torch.float64: 1.43e-15}
MEASURED_RESIDUAL = {torch.float32: 3.76e-5, torch.float64: 1.02e-10}


def value_bound(dt):
    return 4.0 * MEASURED_VALUE_ERROR[dt]


def residual_bound(dt):
    return 4.0 * MEASURED_RESIDUAL[dt]


# ------------------------------------------------------------------ cases
@functools.lru_cache(maxsize=None)
def case(name, dt):
    """(cast cores on the CPU, dims, dense fp64 matrix of the CAST cores, its eigenvalues, its eigenvectors)."""
    cores, dims = MATRICES[name]
    G = [g.to(dt) for g in cores]
    D = dense_matrix(G)
    w, V = torch.linalg.eigh(D)
    return G, dims, D, w, V


def matrix(name, dt, device="cpu"):
    import tntorch_amd as tn

    G, dims, _, _, _ = case(name, dt)
    return tn.TTMatrix([g.to(device) for g in G], None, dims, dims)


def truth(name, dt, which):
    _, _, _, w, V = case(name, dt)
    return (float(w[0]), V[:, 0]) if which == "SA" else (float(w[-1]), V[:, -1])


def start(name, dt, ranks, seed=0, device="cpu"):
    """The start tt_eigsh itself would draw for ``ranks_tt=ranks`` after ``torch.manual_seed(seed)``, as an x0 (so that the host
    and the device run from the same train)."""
    import tntorch_amd as tn
    from tntorch_amd.ttsolve import _max_ranks

    dims = MATRICES[name][1]
    N = len(dims)
    want = list(ranks) if hasattr(ranks, "__len__") else [ranks] * (N - 1)
    rk = [max(1, min(int(r), cap)) for r, cap in zip(want, _max_ranks(dims))]
    torch.manual_seed(seed)
    t = tn.rand(dims, ranks_tt=rk) if N > 1 else tn.rand(dims, ranks_tt=[])
    return tn.Tensor([c.to(device=device, dtype=dt) for c in t.cores])


def value_error(name, dt, which, value):
    l, _ = truth(name, dt, which)
    return abs(float(value) - l) / abs(l)


def dense_residual(name, dt, value, x):
    D = case(name, dt)[2]
    xd = dense(x)
    return float((D @ xd - float(value) * xd).norm() / (D @ xd).norm())


def checked_cases():
    """(name, ranks) of the cases whose value and residual are held against the measured bounds."""
    return [(name, FULL_RANKS[name]) for name in MATRICES] + [(name, 1) for name in RANK_ONE]


# ------------------------------------------------------------------ the Ritz step: operands and references
def ritz_sizes(dt):
    """The sizes of the kernel tests: around a pack, a wave and a workgroup, several workgroups, and the first n at which the
    number of partials reaches its cap (a pack is 16 bytes, a further workgroup joins every 1024 packs, the cap is 256)."""
    V = 4 if dt == torch.float32 else 2
    cap_n = (256 - 1) * 1024 * V + 1
    return [1, 3, 255, 256, 257, 1023, 4099], cap_n


def ritz_vectors(n, dt, seed, offset=0):
    """Random independent X, W, P and A X, A W, A P for the diagonal (hence symmetric) A = diag(a), a in [0.5, 2.5), rounded to
    dt; ``offset`` elements of padding in front (views off a 16-byte boundary)."""
    g = torch.Generator().manual_seed(1000 * seed + n % 997)
    draw = lambda: torch.randn(n, dtype=torch.float64, generator=g)  # noqa: E731
    a = 0.5 + 2.0 * torch.rand(n, dtype=torch.float64, generator=g)
    X, W, P = draw(), draw(), draw()
    vs = [X, a * X, W, a * W, P, a * P]
    out = []
    for v in vs:
        buf = torch.zeros(n + offset, dtype=dt)
        buf[offset:] = v.to(dt)
        out.append(buf[offset:])
    return out


def gram64(X, AX, W=None, AW=None, P=None, AP=None):
    """(the twelve sums in fp64, the twelve sums of the absolute products) of CPU copies of the operands; None is a zero."""
    d = lambda v: None if v is None else v.detach().double().cpu()  # noqa: E731
    X, AX, W, AW, P, AP = d(X), d(AX), d(W), d(AW), d(P), d(AP)
    pairs = [(X, X), (X, W), (X, P), (W, W), (W, P), (P, P), (X, AX), (X, AW), (X, AP), (W, AW), (W, AP), (P, AP)]
    zero = torch.zeros((), dtype=torch.float64)
    val = torch.stack([zero if a is None or b is None else (a * b).sum() for a, b in pairs])
    mag = torch.stack([zero if a is None or b is None else (a * b).abs().sum() for a, b in pairs])
    return val, mag

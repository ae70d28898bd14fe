"""What the tests of ``tn.tt_solve``, of its ops (``env_half_apply``, ``local_matvec``, ``env_update``) and of the kernel behind
them, ``ttr_env_half_apply``, share.  Cores are built by hand in torch; every truth is dense fp64 (``torch.linalg.solve``,
``torch.einsum``) and independent of the package.

The kernel's bound.  H[r, i, c, s] = sum_k G_k T_k with k = (a, j) and T_k = sum_b Phi[r, a, b] X[b, j, s].  The kernel computes
T_k as an fma chain of R' terms (quads, zero-padded: a zero term adds no error) and H as an fma chain of A J terms over the
ROUNDED T_k.  With u the unit roundoff and gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability, section 3.1):
    |That_k - T_k| <= gamma_R' sum_b |Phi||X|,    |Hhat - sum_k G_k That_k| <= gamma_AJ sum_k |G_k||That_k|
so  |Hhat - H| <= (gamma_AJ + gamma_R' + gamma_AJ gamma_R') half_apply(|Phi|, |X|, |G|) <= 2 (R' + A J + 2) u half_apply(|Phi|, |X|, |G|)
for every size tested here (n u << 1: the factor 2 covers the denominators and the product term).  A GEMM over K further terms
on top (the local matvec: K = A' S'; an environment update: K = R I) adds gamma_K of the same magnitude product:
    2 (R' + A J + K + 3) u * (the contraction of the absolute values).
"""
import functools
import math

import torch

DTYPES = [torch.float32, torch.float64]


def unit(dtype):
    return 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53


# ------------------------------------------------------------------ the kernel
# (R, A, R', J, S', I, A').  Tiles: 16 r x 16 s' x 64 columns (i, a'), k = (a, j) in chunks of 16, r' in quads.
SHAPES = [
    (1, 1, 1, 1, 1, 1, 1),        # every extent 1
    (1, 1, 1, 5, 7, 5, 3),        # a first site: R = A = R' = 1
    (6, 3, 5, 4, 1, 4, 1),        # a last site: S' = A' = 1
    (5, 2, 7, 3, 6, 3, 2),        # J and R' no multiples of 4
    (3, 5, 4, 1, 3, 2, 2),        # J = 1
    (3, 2, 4, 3, 5, 1, 6),        # I = 1
    (2, 3, 15, 5, 3, 2, 2),       # R' and A J one below the chunk of 16
    (2, 2, 16, 8, 3, 2, 2),       # at it
    (2, 1, 17, 17, 3, 2, 2),      # one above (A = 1)
    (3, 1, 31, 31, 5, 2, 3),      # R' and A J at 31 / 32 / 33: two chunks
    (4, 4, 32, 8, 3, 3, 2),
    (2, 3, 33, 11, 4, 2, 2),
    (15, 2, 3, 3, 17, 2, 2),      # rows: R and S' one below, at and one above the tile of 16
    (16, 1, 4, 4, 16, 3, 1),
    (17, 2, 2, 2, 15, 2, 3),
    (2, 2, 3, 2, 3, 5, 3),        # columns I A' = 15
    (2, 2, 3, 2, 3, 4, 4),        # 16
    (2, 2, 3, 2, 3, 17, 1),       # 17
    (2, 2, 3, 2, 3, 9, 7),        # 63: one below the column tile
    (2, 2, 3, 2, 3, 8, 8),        # 64
    (2, 2, 3, 2, 3, 13, 5),       # 65
    (33, 2, 9, 6, 35, 10, 13),    # three tiles along r, s' and the columns; 150150 outputs
]
assert all(s[0] * s[5] * s[6] * s[4] < 10 ** 6 for s in SHAPES)
assert all(any(s[ax] == 1 for s in SHAPES) for ax in range(7))


def operands(shape, dtype, seed=5):
    """Phi [R, A, R'], X [R', J, S'], G [A, I, J, A'] drawn in fp64 and rounded to dtype (CPU, contiguous)."""
    R, A, Rp, J, Sp, I, Ap = shape
    g = torch.Generator().manual_seed(seed + sum(shape))
    draw = lambda *s: torch.randn(s, dtype=torch.float64, generator=g).to(dtype)  # noqa: E731
    return draw(R, A, Rp), draw(Rp, J, Sp), draw(A, I, J, Ap)


def half_apply64(Phi, X, G):
    return torch.einsum("rab,bjs,aijc->rics", Phi.double().cpu(), X.double().cpu(), G.double().cpu())


def half_truth_and_bound(Phi, X, G, dtype):
    """(H64, bound) from the operands as given (cast to fp64): the bound of the module docstring."""
    Rp, AJ = Phi.shape[2], Phi.shape[1] * X.shape[1]
    return half_apply64(Phi, X, G), 2 * (Rp + AJ + 2) * unit(dtype) * half_apply64(Phi.abs(), X.abs(), G.abs())


def matvec64(Phi, G, Psi, v):
    return torch.einsum("rab,aijc,tcs,bjs->rit", Phi.double().cpu(), G.double().cpu(), Psi.double().cpu(), v.double().cpu())


def matvec_truth_and_bound(Phi, G, Psi, v, dtype):
    terms = Phi.shape[2] + Phi.shape[1] * v.shape[1] + Psi.shape[1] * Psi.shape[2] + 3
    return matvec64(Phi, G, Psi, v), 2 * terms * unit(dtype) * matvec64(Phi.abs(), G.abs(), Psi.abs(), v.abs())


def env64(side, env, G, bra, ket):
    env, G, bra, ket = env.double().cpu(), G.double().cpu(), bra.double().cpu(), ket.double().cpu()
    if side == "left":
        return torch.einsum("rab,rit,aijc,bjs->tcs", env, bra, G, ket)
    return torch.einsum("tcs,rit,aijc,bjs->rab", env, bra, G, ket)


def env_truth_and_bound(side, env, G, bra, ket, dtype):
    """The four-operand einsum and its bound: the kernel's two chains and the GEMM over (r, i) resp. (s, i)."""
    if side == "left":
        terms = env.shape[2] + env.shape[1] * ket.shape[1] + bra.shape[0] * bra.shape[1] + 3
    else:
        terms = env.shape[2] + env.shape[1] * ket.shape[1] + bra.shape[2] * bra.shape[1] + 3
    return env64(side, env, G, bra, ket), 2 * terms * unit(dtype) * env64(side, env.abs(), G.abs(), bra.abs(), ket.abs())


def assert_within(out, ref, bound, what=""):
    out = out.detach().double().cpu()
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    err = (out - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print("{}: largest error / bound = {:.3f}".format(what, worst))
    assert bool((err <= bound).all()), "{}: error reaches {:.3f} of the bound".format(what, worst)


# ------------------------------------------------------------------ matrices (fp64 cores [a, i, j, a'], symmetric in (i, j))
def _lap(n):
    return 2.0 * torch.eye(n, dtype=torch.float64) - torch.diag(torch.ones(n - 1, dtype=torch.float64), 1) - torch.diag(
        torch.ones(n - 1, dtype=torch.float64), -1)


def kron_cores(dims, seed=21):
    """Rank 1: factor k is I + 0.25 B / ||B||_2 with B a random symmetric matrix (eigenvalues in [0.75, 1.25])."""
    g = torch.Generator().manual_seed(seed)
    cores = []
    for n in dims:
        B = torch.randn((n, n), dtype=torch.float64, generator=g)
        B = B + B.t()
        cores.append((torch.eye(n, dtype=torch.float64) + 0.25 * B / torch.linalg.matrix_norm(B, 2))[None, :, :, None])
    return cores


def laplace_cores(dims, shift=1.0, c=0.25):
    """shift I + c sum_k L_k with L = tridiag(-1, 2, -1), as the rank-2 TT-matrix [c L, I] ... [[I, 0], [c L, I]] ... [I; c L + shift I]."""
    N, cores = len(dims), []
    for k, n in enumerate(dims):
        I, L = torch.eye(n, dtype=torch.float64), c * _lap(n)
        if N == 1:
            cores.append((shift * I + L)[None, :, :, None])
        elif k == 0:
            cores.append(torch.stack([L, I], dim=-1)[None])
        elif k == N - 1:
            cores.append(torch.stack([I, L + shift * I], dim=0)[..., None])
        else:
            G = torch.zeros((2, n, n, 2), dtype=torch.float64)
            G[0, :, :, 0], G[1, :, :, 0], G[1, :, :, 1] = I, L, I
            cores.append(G)
    return cores


def shifted_cores(dims, seed=22, r=2):
    """I + 0.5 S: S a random TT-matrix of rank r whose slices are symmetrised and scaled by 1 / (n sqrt(r)), as block cores of
    rank 1 + r (the identity's rank-1 cores beside those of S)."""
    g = torch.Generator().manual_seed(seed)
    N, cores = len(dims), []
    rk = [1] + [r] * (N - 1) + [1]
    for k, n in enumerate(dims):
        S = torch.randn((rk[k], n, n, rk[k + 1]), dtype=torch.float64, generator=g)
        S = (S + S.permute(0, 2, 1, 3)) / 2 / (n * math.sqrt(r))
        if k == 0:
            S = 0.5 * S
        I = torch.eye(n, dtype=torch.float64)[None, :, :, None]
        if N == 1:
            cores.append(I + S)
            continue
        G = torch.zeros((1 if k == 0 else 1 + r, n, n, 1 if k == N - 1 else 1 + r), dtype=torch.float64)
        G[:1, :, :, :1] = I
        G[(0 if k == 0 else 1):, :, :, (0 if k == N - 1 else 1):] = S
        cores.append(G)
    return cores


MATRICES = {
    "kron": (kron_cores, [4, 3, 5]),
    "laplace": (laplace_cores, [4, 3, 5]),
    "laplace4": (laplace_cores, [3, 4, 2, 5]),
    "shifted": (shifted_cores, [4, 3, 5]),
}
FULL_RANKS = {"kron": [4, 5], "laplace": [4, 5], "laplace4": [3, 10, 5], "shifted": [4, 5]}
COND_LIMITS = {"kron": 5.0, "laplace": 2.83, "laplace4": 2.86, "shifted": 1.5}   # laplace: 2.82 and 2.85 (printed below)


def dense_matrix(cores):
    """The dense [prod I, prod J] matrix of TT-matrix cores [a, i, j, a'] in fp64, by plain contraction."""
    acc = torch.ones((1, 1, 1), dtype=torch.float64)
    for G in cores:
        G = G.double().cpu()
        acc = torch.einsum("xya,aijb->xiyjb", acc, G).reshape(acc.shape[0] * G.shape[1], acc.shape[1] * G.shape[2], G.shape[3])
    return acc[:, :, 0]


def dense_train(cores):
    """The dense vector of TT cores [a, n, b] in fp64."""
    acc = torch.ones((1, 1), dtype=torch.float64)
    for c in cores:
        c = c.double().cpu()
        acc = torch.einsum("xa,anb->xnb", acc, c).reshape(-1, c.shape[2])
    return acc[:, 0]


def train_cores(dims, ranks, seed):
    g = torch.Generator().manual_seed(seed)
    rk = [1] + list(ranks) + [1]
    return [torch.randn((rk[k], n, rk[k + 1]), dtype=torch.float64, generator=g) for k, n in enumerate(dims)]


def product_cores(mcores, xcores):
    """The unrounded cores of A x for a symmetric A: b_k[(r, a), i, (s, a')] = sum_j x[r, j, s] A[a, i, j, a']."""
    out = []
    for G, x in zip(mcores, xcores):
        c = torch.einsum("rjs,aijc->raisc", x, G)
        out.append(c.reshape(x.shape[0] * G.shape[0], G.shape[1], x.shape[2] * G.shape[3]))
    return out


@functools.lru_cache(maxsize=None)
def matrix(name):
    """(fp64 cores, dims, dense fp64 matrix, condition number); symmetry and the condition number are asserted."""
    build, dims = MATRICES[name]
    cores = build(dims)
    D = dense_matrix(cores)
    assert float((D - D.t()).abs().max()) <= 1e-15 * float(D.abs().max()), name
    w = torch.linalg.eigvalsh(D)
    cond = float(w[-1] / w[0])
    print("solve_cases: {} {}: eigenvalues in [{:.4f}, {:.4f}], condition number {:.3f}".format(name, dims, float(w[0]), float(w[-1]), cond))
    assert float(w[0]) > 0 and cond <= COND_LIMITS[name], (name, cond)
    return cores, dims, D, cond


@functools.lru_cache(maxsize=None)
def system(name, rhs):
    """(matrix cores, dims, dense matrix, cond, b cores, dense b, dense solution, x_true cores or None), all fp64.
    ``rhs == "random"``: a random rank-2 train; ``rhs == "product"``: b = A x_true, the unrounded product cores of a rank-2 x_true."""
    cores, dims, D, cond = matrix(name)
    ranks = [2] * (len(dims) - 1)
    if rhs == "random":
        xt, bc = None, train_cores(dims, ranks, 31)
    else:
        xt = train_cores(dims, ranks, 32)
        bc = product_cores(cores, xt)
    bd = dense_train(bc)
    xd = torch.linalg.solve(D, bd)
    if xt is not None:
        assert float((dense_train(xt) - xd).norm()) <= 1e-12 * float(xd.norm())
    return cores, dims, D, cond, bc, bd, xd, xt


def start_cores(dims, seed):
    """A rank-2 start for the rank-2 systems."""
    return train_cores(dims, [2] * (len(dims) - 1), 100 + seed)


def energy(D, bd, xd):
    """x^T A x / 2 - b^T x in fp64."""
    return float(xd @ (D @ xd) / 2 - bd @ xd)


# ------------------------------------------------------------------ what the host and the device tests of tt_solve share
TOL = {torch.float32: None, torch.float64: 1e-9}


def tol_of(dt):
    return math.sqrt(torch.finfo(dt).eps) if TOL[dt] is None else TOL[dt]


def build(name, rhs, dt, device="cpu"):
    """(TTMatrix, b, dense fp64 matrix, dense fp64 b, dense fp64 solution, cond) of a case, everything from the CAST operands."""
    import tntorch_amd as tn

    cores, dims, _, cond, bc, _, _, _ = system(name, rhs)
    G = [g.to(dt) for g in cores]
    bt = [c.to(dt) for c in bc]
    D, bd = dense_matrix(G), dense_train(bt)
    A = tn.TTMatrix([g.to(device) for g in G], None, dims, dims)
    b = tn.Tensor([c.to(device) for c in bt])
    return A, b, D, bd, torch.linalg.solve(D, bd), cond


def dense(x):
    return dense_train([c.detach().cpu() for c in x.cores])


def rel_residual(D, bd, x):
    return float((D @ dense(x) - bd).norm() / bd.norm())

"""``tn.tt_solve`` on CPU tensors (the host mirror of the device ops), against dense fp64 solves of the same (cast) operands, and
the argument checks of ``ttr_env_half_apply``, which return before anything touches a device.

Tolerances: ``tol`` is 1e-9 in fp64 and the default ``sqrt(eps)`` = 3.45e-4 in fp32.  The local solves go to ``tol / 10``, so
the dense residual ``||A x - b|| / ||b||`` is asserted ``<= tol``, and the error ``||x - x_true|| / ||x_true|| <= cond(A) tol``
follows from it (``x - x_true = A^-1 (A x - b)`` and ``||b|| <= ||A|| ||x_true||``)."""
import ctypes
import math
import os
import re

import pytest
import torch

import solve_cases as sc
import tntorch_amd as tn
from tntorch_amd import _hip, _hipops, _hostops, ttsolve

DTYPES = sc.DTYPES
TOL, tol_of, build, dense, rel_residual = sc.TOL, sc.tol_of, sc.build, sc.dense, sc.rel_residual


# ------------------------------------------------------------------ the mirror ops
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", [(5, 2, 7, 3, 6, 3, 2), (1, 1, 1, 5, 7, 5, 3), (6, 3, 5, 4, 1, 4, 1)])
def test_host_env_half_apply(shape, dt):
    Phi, X, G = sc.operands(shape, dt)
    ref, bound = sc.half_truth_and_bound(Phi, X, G, dt)
    out = _hostops.env_half_apply(Phi, X, G)
    assert out.is_contiguous() and out.dtype == dt
    sc.assert_within(out, ref, bound, "host env_half_apply {} {}".format(shape, dt))
    sc.assert_within(_hostops.env_half_apply(Phi, X.permute(2, 1, 0).contiguous().permute(2, 1, 0),
                                             G.permute(3, 1, 2, 0).contiguous().permute(3, 1, 2, 0)), ref, bound, "host views")


@pytest.mark.parametrize("dt", DTYPES)
def test_host_local_matvec_and_env_update(dt):
    g = torch.Generator().manual_seed(9)
    R, A, I, S = 5, 3, 6, 7
    draw = lambda *s: torch.randn(s, dtype=torch.float64, generator=g).to(dt)  # noqa: E731
    Phi, Psi, G, v, bra = draw(R, A, R), draw(S, A, S), draw(A, I, I, A), draw(R, I, S), draw(R, I, S)
    ref, bound = sc.matvec_truth_and_bound(Phi, G, Psi, v, dt)
    sc.assert_within(_hostops.local_matvec(Phi, G, Psi, v), ref, bound, "host local_matvec")
    for side, env in (("left", Phi), ("right", Psi)):
        ref, bound = sc.env_truth_and_bound(side, env, G, bra, v, dt)
        sc.assert_within(_hostops.env_update(side, env, G, bra, v), ref, bound, "host env_update " + side)
    with pytest.raises(ValueError):
        _hostops.env_update("up", Phi, G, bra, v)


# ------------------------------------------------------------------ the solver
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(sc.MATRICES))
def test_full_ranks_solve_in_one_sweep(name, dt):
    """At full ranks a local solve is a global solve: after the FIRST sweep the dense residual is <= tol, and the second sweep
    sees it and stops."""
    A, b, D, bd, xd, cond = build(name, "random", dt)
    tol = tol_of(dt)
    x1 = tn.tt_solve(A, b, ranks_tt=sc.FULL_RANKS[name], nswp=1, tol=TOL[dt])
    res = rel_residual(D, bd, x1)
    print("full ranks {} {}: dense residual after one sweep {:.3e}".format(name, dt, res))
    assert res <= tol
    x, info = tn.tt_solve(A, b, ranks_tt=99, tol=TOL[dt], return_info=True)
    assert info["converged"] and info["sweeps"] == 2 and len(info["local_residuals"]) == 2
    assert info["local_residuals"][1] <= tol < info["local_residuals"][0]
    assert [int(r) for r in x.ranks_tt] == [1] + sc.FULL_RANKS[name] + [1]
    res = rel_residual(D, bd, x)
    assert res <= tol and abs(info["residual"] - res) <= 0.05 * res + 64 * sc.unit(dt)
    assert float((dense(x) - xd).norm() / xd.norm()) <= cond * tol
    assert all(c.dtype == dt and not c.requires_grad for c in x.cores)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("name", ["laplace", "laplace4", "shifted"])
def test_rank_two_systems(name, seed, dt):
    """b = A x_true with a rank-2 x_true, from a random rank-2 x0: the energy x^T A x / 2 - b^T x (dense, fp64) never increases
    from sweep to sweep beyond 8 u |E|, the run converges within 20 sweeps, the dense residual is <= tol and the error
    <= cond(A) tol."""
    A, b, D, bd, xd, cond = build(name, "product", dt)
    tol, dims = tol_of(dt), sc.MATRICES[name][1]
    x0 = tn.Tensor([c.to(dt) for c in sc.start_cores(dims, seed)])
    keep = [c.clone() for c in x0.cores]
    x, info = tn.tt_solve(A, b, x0=x0, tol=TOL[dt], return_info=True)
    assert all(torch.equal(a, c) for a, c in zip(keep, x0.cores))
    assert info["converged"] and info["sweeps"] <= 20 and len(info["local_residuals"]) == info["sweeps"]
    assert [int(r) for r in x.ranks_tt] == [int(r) for r in x0.ranks_tt]
    res = rel_residual(D, bd, x)
    err = float((dense(x) - xd).norm() / xd.norm())
    print("rank 2 {} seed {} {}: {} sweeps, dense residual {:.3e}, error {:.3e}".format(name, seed, dt, info["sweeps"], res, err))
    assert res <= tol and err <= cond * tol
    energies = [sc.energy(D, bd, dense(x0))]
    for s in range(1, info["sweeps"] + 1):
        energies.append(sc.energy(D, bd, dense(tn.tt_solve(A, b, x0=x0, nswp=s, tol=TOL[dt]))))
    for before, after in zip(energies, energies[1:]):
        assert after <= before + 8 * sc.unit(dt) * abs(before), energies
    assert abs(energies[-1] - sc.energy(D, bd, dense(x))) <= 8 * sc.unit(dt) * abs(energies[-1])


@pytest.mark.parametrize("dt", DTYPES)
def test_kron_rank_one(dt):
    """A rank-1 matrix and a rank-1 b: with ranks_tt=1 one sweep returns the Kronecker product of the factor solves."""
    cores, dims, _, cond = sc.matrix("kron")
    G = [g.to(dt) for g in cores]
    bc = [c.to(dt) for c in sc.train_cores(dims, [1, 1], 33)]
    D, bd = sc.dense_matrix(G), sc.dense_train(bc)
    want = None
    for g, c in zip(G, bc):
        f = torch.linalg.solve(g[0, :, :, 0].double(), c[0, :, 0].double())
        want = f if want is None else torch.kron(want, f)
    x, info = tn.tt_solve(tn.TTMatrix(G, None, dims, dims), tn.Tensor(bc), ranks_tt=1, nswp=1, tol=TOL[dt], return_info=True)
    res = rel_residual(D, bd, x)
    print("kron rank 1 {}: dense residual {:.3e}".format(dt, res))
    assert info["sweeps"] == 1 and not info["converged"] and res <= tol_of(dt)
    assert float((dense(x) - want).norm() / want.norm()) <= cond * tol_of(dt)


@pytest.mark.parametrize("dt", DTYPES)
def test_transpose_zero_single_mode_and_info(dt):
    A, b, D, bd, xd, cond = build("shifted", "random", dt)
    tol = tol_of(dt)
    x = tn.tt_solve(A, b, ranks_tt=[4, 5], tol=TOL[dt])
    xt = tn.tt_solve(A, b, transpose=True, ranks_tt=[4, 5], tol=TOL[dt])
    assert float((dense(x) - dense(xt)).norm() / xd.norm()) <= 2 * cond * tol      # a symmetric matrix: the two forms coincide
    assert rel_residual(D, bd, xt) <= tol
    # N = 1: a single local solve per sweep
    n = 5
    L = (torch.eye(n, dtype=torch.float64) * 2 + torch.tril(torch.ones(n, n, dtype=torch.float64), -1) * 0.1).to(dt)
    S = (L @ L.t())  # SPD, for the solver
    bv = torch.arange(1, n + 1, dtype=dt)
    As, b1 = tn.TTMatrix([S[None, :, :, None]], None, [n], [n]), tn.Tensor([bv[None, :, None]])
    x1, info = tn.tt_solve(As, b1, ranks_tt=1, tol=TOL[dt], return_info=True)
    assert sorted(info) == ["converged", "local_residuals", "residual", "sweeps"]
    assert info["converged"] and info["sweeps"] == 2 and isinstance(info["residual"], float)
    assert all(isinstance(v, float) for v in info["local_residuals"])
    assert float((S.double() @ x1.torch().double() - bv.double()).norm() / bv.double().norm()) <= tol
    # b == 0: the rank-1 zero train, no sweep
    zero = tn.Tensor([torch.zeros_like(c) for c in b.cores])
    before = dict(ttsolve.READBACKS)
    z, info = tn.tt_solve(A, zero, ranks_tt=3, return_info=True)
    assert [int(r) for r in z.ranks_tt] == [1, 1, 1, 1] and float(z.torch().abs().max()) == 0.0 and z.cores[0].dtype == dt
    assert info["sweeps"] == 0 and info["local_residuals"] == [] and info["residual"] == 0.0
    assert ttsolve.READBACKS["sweep"] == before["sweep"]


def test_one_readback_per_sweep_and_verbose(capsys):
    A, b, D, bd, xd, cond = build("laplace", "product", torch.float64)
    before = dict(ttsolve.READBACKS)
    x, info = tn.tt_solve(A, b, ranks_tt=2, tol=1e-9, verbose=True, return_info=True)
    assert ttsolve.READBACKS["sweep"] - before["sweep"] == info["sweeps"]
    assert ttsolve.READBACKS["setup"] - before["setup"] == 1 and ttsolve.READBACKS["residual"] - before["residual"] == 1
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("tt_solve: sweep")]
    assert len(lines) == info["sweeps"]


def test_tucker_factors_and_grad_operands_on_the_cpu():
    """Tucker factors of b and x0 are contracted in; the call runs under no_grad and returns detached cores."""
    dt = torch.float64
    A, b, D, bd, xd, cond = build("laplace", "product", dt)
    dims = sc.MATRICES["laplace"][1]
    g = torch.Generator().manual_seed(5)
    Us = [torch.linalg.qr(torch.randn((n, n), dtype=dt, generator=g))[0] for n in dims]
    bt = tn.Tensor([torch.einsum("anb,nm->amb", c, U) for c, U in zip(b.cores, Us)], Us=[U.clone() for U in Us])
    assert float((bt.torch() - b.torch()).abs().max()) <= 1e-12
    x0 = tn.Tensor([c.to(dt) for c in sc.start_cores(dims, 0)])
    x0t = tn.Tensor([torch.einsum("anb,nm->amb", c, U) for c, U in zip(x0.cores, Us)], Us=[U.clone() for U in Us])
    x = tn.tt_solve(A, bt, x0=x0t, tol=1e-9)
    assert rel_residual(D, bd, x) <= 1e-9 and all(U is None for U in x.Us)
    for c in A.cores + b.cores:
        c.requires_grad_(True)
    y = tn.tt_solve(A, b, x0=x0, tol=1e-9)
    assert all(not c.requires_grad and c.grad_fn is None for c in y.cores) and rel_residual(D, bd, y) <= 1e-9


def test_an_indefinite_matrix_is_refused():
    dims = [4, 3, 5]
    G = sc.laplace_cores(dims, shift=1.0 - 3.0)      # "laplace" with the shift -3 I: eigenvalues of both signs
    w = torch.linalg.eigvalsh(sc.dense_matrix(G))
    assert float(w[0]) < 0 < float(w[-1])
    b = tn.Tensor(sc.train_cores(dims, [2, 2], 31))
    with pytest.raises(ValueError, match="not positive definite"):
        tn.tt_solve(tn.TTMatrix(G, None, dims, dims), b, ranks_tt=[4, 5], tol=1e-9)


def test_refusals():
    dt = torch.float64
    A, b, *_ = build("laplace", "random", dt)
    dims = sc.MATRICES["laplace"][1]
    ok = dict(ranks_tt=2)
    with pytest.raises(ValueError, match="must be a TTMatrix"):
        tn.tt_solve(b, b, **ok)
    with pytest.raises(ValueError, match="b must be a tntorch_amd.Tensor"):
        tn.tt_solve(A, b.torch(), **ok)
    with pytest.raises(ValueError, match="x0 must be a tntorch_amd.Tensor"):
        tn.tt_solve(A, b, x0=b.torch())
    with pytest.raises(ValueError, match="batched"):
        tn.tt_solve(tn.TTMatrix([c[None] for c in A.cores], None, dims, dims), b, **ok)
    with pytest.raises(ValueError, match="batched"):
        tn.tt_solve(A, tn.Tensor([c[None] for c in b.cores], batch=True), **ok)
    with pytest.raises(ValueError, match="boundary ranks"):
        tn.tt_solve(tn.TTMatrix([torch.cat([A.cores[0]] * 2, dim=0)] + A.cores[1:], None, dims, dims), b, **ok)
    with pytest.raises(ValueError, match="boundary ranks of b"):
        tn.tt_solve(A, tn.Tensor([torch.cat([b.cores[0]] * 2, dim=0)] + b.cores[1:]), **ok)
    with pytest.raises(ValueError, match="3 modes, b has 2"):
        tn.tt_solve(A, tn.Tensor([b.cores[0], b.cores[1][:, :, :1]]), **ok)
    wide = [A.cores[0], A.cores[1][:, :, :2], A.cores[2]]
    with pytest.raises(ValueError, match="mode 1 of the matrix is not square"):
        tn.tt_solve(tn.TTMatrix(wide, None, dims, [4, 2, 5]), b, **ok)
    with pytest.raises(ValueError, match="mode 2 of b has size 4"):
        tn.tt_solve(A, tn.Tensor([b.cores[0], b.cores[1], b.cores[2][:, :4]]), **ok)
    with pytest.raises(ValueError, match="mode 0 of x0 has size 3"):
        tn.tt_solve(A, b, x0=tn.Tensor([b.cores[0][:, :3], b.cores[1], b.cores[2]]))
    with pytest.raises(ValueError, match="float32 or float64"):
        tn.tt_solve(tn.TTMatrix([c.half() for c in A.cores], None, dims, dims), tn.Tensor([c.half() for c in b.cores]), **ok)
    with pytest.raises(ValueError, match="same dtype"):
        tn.tt_solve(A, tn.Tensor([c.float() for c in b.cores]), **ok)
    with pytest.raises(ValueError, match="same dtype"):
        tn.tt_solve(A, b, x0=tn.Tensor([c.float() for c in b.cores]))
    with pytest.raises(ValueError, match="x0 or ranks_tt"):
        tn.tt_solve(A, b)
    for bad in (dict(nswp=0), dict(local_iters=0), dict(tol=0.0), dict(tol=-1e-3)):
        with pytest.raises(ValueError, match="nswp and local_iters|tol must be positive"):
            tn.tt_solve(A, b, **ok, **bad)
    with pytest.raises(NotImplementedError, match="CP cores"):
        tn.tt_solve(A, tn.Tensor([torch.rand(n, 2, dtype=dt) for n in dims]), **ok)


# ------------------------------------------------------------------ the C ABI's refusals
INVALID, UNSUPPORTED = -1, -2
_BUF = [(ctypes.c_double * 512)() for _ in range(4)]
P0, P1, P2, P3 = (ctypes.addressof(x) for x in _BUF)


def _i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


def half(dtype=0, R=5, A=2, Rp=7, J=3, Sp=6, I=3, Ap=2, Phi=P0, X=P1, xs=(18, 6, 1), G=P2, gs=(18, 6, 2, 1), H=P3):
    return (dtype, R, A, Rp, J, Sp, I, Ap, Phi, X, None if xs is None else _i64(*xs), G, None if gs is None else _i64(*gs), H, None)


REFUSALS = [
    (half(dtype=7), INVALID, "ttr_env_half_apply: bad dtype 7"),
] + [
    (half(**{name: 0}), INVALID, "ttr_env_half_apply: bad sizes") for name in ("R", "A", "Rp", "J", "Sp", "I", "Ap")
] + [
    (half(J=-2), INVALID, "ttr_env_half_apply: bad sizes Phi [5, 2, 7], X [7, -2, 6], G [2, 3, -2, 2]"),
] + [
    (half(**{name: None}), INVALID, "ttr_env_half_apply: null pointer") for name in ("Phi", "X", "xs", "G", "gs", "H")
] + [
    (half(H=p), INVALID, "ttr_env_half_apply: H must not be an input") for p in (P0, P1, P2)
] + [
    (half(xs=(18, -6, 1)), UNSUPPORTED, "X [R', J, S'] needs non-negative element strides"),
    (half(gs=(18, 6, 2, -1)), UNSUPPORTED, "G [A, I, J, A'] needs non-negative element strides"),
    (half(xs=(1 << 56, 6, 1)), UNSUPPORTED, "X [R', J, S'] needs non-negative element strides"),
    (half(gs=(1, 1, 1, 1 << 57)), UNSUPPORTED, "G [A, I, J, A'] needs non-negative element strides"),
    (half(J=1 << 31), UNSUPPORTED, "an extent does not fit 32 bits"),
    (half(A=1 << 16, J=1 << 16), UNSUPPORTED, "A J and I A' must be at most 2^31 - 1"),
    (half(I=1 << 20, Ap=1 << 11), UNSUPPORTED, "A J and I A' must be at most 2^31 - 1"),
    (half(R=1 << 20, A=1 << 20, Rp=1 << 20), UNSUPPORTED, "operand too large"),
    (half(R=1 << 20, I=1 << 15, Ap=1 << 15, Sp=1 << 20), UNSUPPORTED, "operand too large"),
    # 2^26 x 2^4 x 2^9 tiles of a result of 2^56 elements
    (half(R=1 << 30, I=1 << 15, Ap=1, Sp=1 << 8, Rp=1, A=1), UNSUPPORTED, "workgroups do not fit a 32-bit grid"),
]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()  # hipcc cross-compiles gfx950 without a GPU
    L = ctypes.CDLL(g.LIB)
    for name, (res, args) in _hip._SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L


@pytest.mark.skipif(torch.cuda.is_available(), reason="host addresses must not reach a launch on a real device")
@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_cabi_refusal(lib, case):
    """The checks return before anything touches a device: the library is called with the addresses of small host arrays."""
    args, status, text = REFUSALS[case]
    assert lib.ttr_env_half_apply(*args) == status
    assert text in lib.ttr_last_error().decode()


# ------------------------------------------------------------------ wiring
def test_wiring():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert tn.ttsolve.__all__ == ["tt_solve"] and tn.tt_solve is tn.ttsolve.tt_solve
    header = open(os.path.join(root, "include", "ttround_hip.h")).read()
    above, below = header.split("#define TTR_ABI_VERSION")
    assert "ttr_env_half_apply" in above and _hip.ABI_VERSION == 17
    assert re.search(r"\bint\s+ttr_env_half_apply\s*\(\s*int dtype, int64_t R, int64_t A, int64_t Rp, int64_t J, int64_t Sp, int64_t I,\s*"
                     r"int64_t Ap,\s*const void\* Phi,\s*const void\* X, const int64_t\* x_strides, const void\* G,\s*"
                     r"const int64_t\* g_strides,\s*void\* H, void\* stream\)", below)
    assert "ttr_env_half_apply" in _hip.EXPORTED_SYMBOLS
    assert (_hip.ENV_TILE_R, _hip.ENV_TILE_S, _hip.ENV_TILE_N, _hip.ENV_TILE_K) == (16, 16, 64, 16)
    makefile = open(os.path.join(root, "tntorch_amd", "csrc", "Makefile")).read()
    assert re.search(r"^  ttr_ttsolve\.hip \\$", makefile, flags=re.M)
    for mod in (_hipops, _hostops):
        assert all(callable(getattr(mod, n)) for n in ("env_half_apply", "env_half_apply_unfused", "local_matvec", "env_update", "gemm2d"))
    assert callable(_hip.env_half_apply)
    assert "## 29." in open(os.path.join(root, "DESIGN.md")).read()
    assert "tt_solve" in open(os.path.join(root, "README.md")).read() and "tt_solve" in tn.__doc__

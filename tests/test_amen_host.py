"""``tn.tt_amen_solve`` on CPU tensors (the host mirror of the device ops), against dense fp64 solves of the same (cast) operands;
the mirror of the fused CG step against ``ttsolve._cg``; and the argument checks of ``ttr_cg_*``, which return before anything
touches a device.

Tolerances: ``tol = solve_cases.tol_of(dt)``; the local solves go to ``tol / 10``, the truncations and the final rounding to
``eps = tol / 10``.  The dense residual is asserted ``<= (1 + cond / 10) tol`` (``amen_cases.residual_bound``)."""
import ctypes
import os
import re

import pytest
import torch

import amen_cases as ac
import solve_cases as sc
import tntorch_amd as tn
from tntorch_amd import _hip, _hipops, _hostops, ttamen, ttsolve

DTYPES = sc.DTYPES


def solve(name, rhs, dt, **kw):
    A, b, D, bd, _, cond = sc.build(name, rhs, dt)
    kw.setdefault("tol", sc.tol_of(dt))
    x, info = tn.tt_amen_solve(A, b, return_info=True, **kw)
    return x, info, D, bd, cond


# ------------------------------------------------------------------ the solver
@pytest.mark.parametrize("kick", ac.KICKS)
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name,rhs", ac.SYSTEMS)
def test_converges_from_rank_one(name, rhs, dt, kick):
    x, info, D, bd, cond = solve(name, rhs, dt, kickrank=kick)
    ac.check_solution(name, rhs, kick, x, info, D, bd, cond, sc.tol_of(dt))
    assert all(not c.requires_grad and c.dtype == dt for c in x.cores)
    assert abs(info["residual"] - sc.rel_residual(D, bd, x)) <= 1e-3 * sc.tol_of(dt)


def test_rank_adaptation_is_real():
    """Without enrichment the ranks cannot grow from the rank-1 start; with it the same call converges."""
    _, stuck, _, _, _ = solve("laplace4", "random", torch.float64, kickrank=0, nswp=4)
    assert not stuck["converged"] and stuck["sweeps"] == 4 and all(r == [1, 1, 1] for r in stuck["ranks"])
    x, info, D, bd, cond = solve("laplace4", "random", torch.float64, kickrank=2, nswp=20)
    assert info["converged"] and max(info["ranks"][-1]) > 1
    assert sc.rel_residual(D, bd, x) <= ac.residual_bound(cond, sc.tol_of(torch.float64))


@pytest.mark.parametrize("dt", DTYPES)
def test_determinism_and_seeds(dt):
    x1, i1, D, bd, cond = solve("shifted", "random", dt)
    x2, i2, _, _, _ = solve("shifted", "random", dt)
    assert all(torch.equal(a, b) for a, b in zip(x1.cores, x2.cores)) and i1 == i2
    x3, i3, _, _, _ = solve("shifted", "random", dt, seed=5)
    assert i3["converged"] and sc.rel_residual(D, bd, x3) <= ac.residual_bound(cond, sc.tol_of(dt))
    assert not all(a.shape == b.shape and torch.equal(a, b) for a, b in zip(x1.cores, x3.cores))


@pytest.mark.parametrize("dt", DTYPES)
def test_bookkeeping(dt):
    tol = sc.tol_of(dt)
    A, b, D, bd, _, cond = sc.build("laplace", "random", dt)
    dims = sc.MATRICES["laplace"][1]
    # x0 is never written, and the readbacks are counted
    x0 = tn.Tensor([c.to(dt) for c in sc.start_cores(dims, 1)])
    keep = [c.clone() for c in x0.cores]
    before = dict(ttamen.READBACKS)
    x, info = tn.tt_amen_solve(A, b, x0=x0, tol=tol, return_info=True)
    assert all(torch.equal(a, c) for a, c in zip(keep, x0.cores)) and info["converged"]
    assert sc.rel_residual(D, bd, x) <= ac.residual_bound(cond, tol)
    delta = {k: ttamen.READBACKS[k] - before[k] for k in before}
    assert delta == {"setup": 1, "sweep": info["sweeps"], "residual": 1, "round": 1}
    before = dict(ttamen.READBACKS)
    tn.tt_amen_solve(A, b, tol=tol, nswp=2)
    assert ttamen.READBACKS["residual"] == before["residual"] and ttamen.READBACKS["sweep"] - before["sweep"] <= 2
    # rmax caps every rank of every sweep, and the returned ones
    x, info = tn.tt_amen_solve(A, b, rmax=3, tol=tol, nswp=3, return_info=True)
    assert all(r <= 3 for ranks in info["ranks"] for r in ranks) and all(int(r) <= 3 for r in x.ranks_tt)
    # transpose=True on a symmetric matrix: the same system
    xt, it = tn.tt_amen_solve(A, b, transpose=True, tol=tol, return_info=True)
    assert it["converged"] and sc.rel_residual(D, bd, xt) <= ac.residual_bound(cond, tol)
    # b == 0: the rank-1 zero train
    z, iz = tn.tt_amen_solve(A, tn.Tensor([torch.zeros_like(c) for c in b.cores]), return_info=True)
    assert [tuple(c.shape) for c in z.cores] == [(1, n, 1) for n in dims] and all(float(c.abs().max()) == 0 for c in z.cores)
    assert iz["converged"] and iz["sweeps"] == 0 and iz["residual"] == 0.0
    # one mode: a single local solve per sweep
    M1 = sc.dense_matrix(sc.laplace_cores([6])).to(dt)
    b1 = torch.arange(1.0, 7.0, dtype=dt)
    x1, i1 = tn.tt_amen_solve(tn.TTMatrix([M1[None, :, :, None]], None, [6], [6]), tn.Tensor([b1[None, :, None]]), tol=tol,
                              return_info=True)
    assert i1["converged"] and i1["ranks"] == [[]] * i1["sweeps"]
    assert float((M1.double() @ x1.cores[0].reshape(-1).double() - b1.double()).norm() / b1.double().norm()) <= tol


def test_indefinite_matrix_raises():
    cores = sc.kron_cores([4, 3, 5])
    cores[1] = -cores[1]
    A = tn.TTMatrix(cores, None, [4, 3, 5], [4, 3, 5])
    b = tn.Tensor(sc.train_cores([4, 3, 5], [2, 2], 31))
    with pytest.raises(ValueError, match="not positive definite"):
        tn.tt_amen_solve(A, b)


def test_refusals():
    """Every refusal of tt_amen_solve; the operand checks are tt_solve's (shared code): the same class and message but for the name."""
    dt = torch.float64
    A, b, *_ = sc.build("laplace", "random", dt)
    dims = sc.MATRICES["laplace"][1]
    shared = [
        (ValueError, "must be a TTMatrix", lambda f, kw: f(b, b, **kw)),
        (ValueError, "b must be a tntorch_amd.Tensor", lambda f, kw: f(A, b.torch(), **kw)),
        (ValueError, "x0 must be a tntorch_amd.Tensor", lambda f, kw: f(A, b, x0=b.torch())),
        (ValueError, "batched", lambda f, kw: f(tn.TTMatrix([c[None] for c in A.cores], None, dims, dims), b, **kw)),
        (ValueError, "batched", lambda f, kw: f(A, tn.Tensor([c[None] for c in b.cores], batch=True), **kw)),
        (ValueError, "boundary ranks of b", lambda f, kw: f(A, tn.Tensor([torch.cat([b.cores[0]] * 2, dim=0)] + b.cores[1:]), **kw)),
        (ValueError, "3 modes, b has 2", lambda f, kw: f(A, tn.Tensor([b.cores[0], b.cores[1][:, :, :1]]), **kw)),
        (ValueError, "mode 1 of the matrix is not square",
         lambda f, kw: f(tn.TTMatrix([A.cores[0], A.cores[1][:, :, :2], A.cores[2]], None, dims, [4, 2, 5]), b, **kw)),
        (ValueError, "mode 2 of b has size 4", lambda f, kw: f(A, tn.Tensor([b.cores[0], b.cores[1], b.cores[2][:, :4]]), **kw)),
        (ValueError, "mode 0 of x0 has size 3", lambda f, kw: f(A, b, x0=tn.Tensor([b.cores[0][:, :3], b.cores[1], b.cores[2]]))),
        (ValueError, "float32 or float64",
         lambda f, kw: f(tn.TTMatrix([c.half() for c in A.cores], None, dims, dims), tn.Tensor([c.half() for c in b.cores]), **kw)),
        (ValueError, "same dtype", lambda f, kw: f(A, tn.Tensor([c.float() for c in b.cores]), **kw)),
        (ValueError, "same dtype", lambda f, kw: f(A, b, x0=tn.Tensor([c.float() for c in b.cores]))),
        (ValueError, "nswp and local_iters", lambda f, kw: f(A, b, nswp=0, **kw)),
        (ValueError, "nswp and local_iters", lambda f, kw: f(A, b, local_iters=0, **kw)),
        (ValueError, "tol must be positive", lambda f, kw: f(A, b, tol=0.0, **kw)),
        (ValueError, "tol must be positive", lambda f, kw: f(A, b, tol=-1e-3, **kw)),
        (NotImplementedError, "CP cores", lambda f, kw: f(A, tn.Tensor([torch.rand(n, 2, dtype=dt) for n in dims]), **kw)),
    ]
    for cls, text, call in shared:
        for who, f, kw in (("tt_amen_solve", tn.tt_amen_solve, {}), ("tt_solve", tn.tt_solve, dict(ranks_tt=2))):
            with pytest.raises(cls, match=text) as e:
                call(f, kw)
            assert type(e.value) is cls and who in str(e.value)
    assert ttamen._check_system is ttsolve._check_system and ttamen._check_devices is ttsolve._check_devices
    for bad, text in ((dict(kickrank=-1), "kickrank must not be negative"), (dict(rmax=0), "rmax must be at least 1"),
                      (dict(eps=0.0), "eps must be positive"), (dict(eps=-1e-3), "eps must be positive")):
        with pytest.raises(ValueError, match="tt_amen_solve: " + text):
            tn.tt_amen_solve(A, b, **bad)
    with pytest.raises(TypeError):
        tn.tt_amen_solve(A, b, ranks_tt=2)                                     # the ranks are found, not given
    # grad operands on the CPU: the call runs under no_grad and returns detached cores
    Ag = tn.TTMatrix([c.clone().requires_grad_(True) for c in A.cores], None, dims, dims)   # (clones: the cases are cached)
    x = tn.tt_amen_solve(Ag, b, tol=1e-9)
    assert all(not c.requires_grad and c.grad_fn is None for c in x.cores)


# ------------------------------------------------------------------ the mirror of the CG step
class _Dense:
    """The one op ``ttsolve._cg`` asks for, on a dense SPD matrix: the recurrences alone."""

    def __init__(self, B):
        self.B = B

    def local_matvec(self, Phi, Ak, Psi, v):
        return (self.B.to(v.dtype) @ v.reshape(-1)).reshape(v.shape)


@pytest.mark.parametrize("dt", DTYPES)
def test_mirror_follows_cg(dt):
    """Five steps of the three mirror calls in ``dt``: every call within the bounds of ``amen_cases`` of its own inputs, and the
    iterate within ``10 cond u ||v||`` of ``ttsolve._cg`` run in fp64 on the same (cast) operands, the bound the device solve is
    held to."""
    n, steps = 37, 5
    g = torch.Generator().manual_seed(11)
    Q = torch.linalg.qr(torch.randn((n, n), dtype=torch.float64, generator=g))[0]
    B = (Q * torch.linspace(1.0, 3.0, n, dtype=torch.float64)) @ Q.t()
    B = ((B + B.t()) / 2).to(dt)
    cond = float(torch.linalg.cond(B.double()))
    f, x0 = (torch.randn(n, dtype=torch.float64, generator=g).to(dt) for _ in range(2))
    ops64 = _Dense(B.double())
    v = x0.clone()
    r = (f.double() - B.double() @ x0.double()).to(dt)
    p = r.clone()
    state = ac.make_state(float(torch.dot(r.double(), r.double())), 0.0, 0)
    part = torch.zeros((2, _hostops.cg_parts(dt, n)), dtype=torch.float64)
    assert part.numel() * 8 == _hostops.cg_workspace_bytes(dt, n)
    for step in range(steps):
        Bp = (B.double() @ p.double()).to(dt)
        _hostops.cg_dot(p, Bp, part)
        ac.check_dot(p, Bp, part)
        before = ac.snapshot(p=p, Bp=Bp, v=v, r=r, part=part, state=state)
        _hostops.cg_update(step, p, Bp, v, r, part, state)
        assert ac.check_update(step, before, ac.snapshot(p=p, Bp=Bp, v=v, r=r, part=part, state=state))
        before = ac.snapshot(r=r, p=p, part=part, state=state)
        _hostops.cg_direction(step, r, p, part, state)
        ac.check_direction(step, before, ac.snapshot(r=r, p=p, part=part, state=state))
        stat = torch.zeros(2, dtype=torch.float64)
        ref = ttsolve._cg(ops64, None, None, None, f.double(), x0.double(), 0.0, step + 1, stat)
        err = float((v.double() - ref).norm() / ref.norm())
        print("mirror {} step {}: ||v - _cg|| / ||v|| = {:.3e} (bound {:.3e})".format(dt, step + 1, err, 10 * cond * sc.unit(dt)))
        assert err <= 10 * cond * sc.unit(dt) and float(stat[1]) == 0.0
    assert float(state[3]) == 0.0


@pytest.mark.parametrize("dt", DTYPES)
def test_mirror_steps_that_are_not_live(dt):
    """Frozen (rs <= thr2), p^T B p < 0 and p^T B p == 0: no vector changes; the count rises only for an active step."""
    n = 9
    p, Bp, v, r = ac.vectors(n, dt, seed=2)
    for rs, thr2, pBp, bad in ((1.0, 2.0, 3.0, 0), (1.0, 1.0, -3.0, 0), (2.0, 1.0, -3.0, 1), (2.0, 1.0, 0.0, 1), (0.0, 0.0, 0.0, 0)):
        for step in (0, 1):
            state = ac.make_state(rs, thr2, step & 1, bad=4.0)
            part = torch.zeros((2, 3), dtype=torch.float64)
            part[0] = ac.spread(pBp, 3)
            before = ac.snapshot(p=p, Bp=Bp, v=v, r=r, part=part, state=state)
            _hostops.cg_update(step, p, Bp, v, r, part, state)
            after = ac.snapshot(p=p, Bp=Bp, v=v, r=r, part=part, state=state)
            assert not ac.check_update(step, before, after) and float(state[3]) == 4.0 + bad
            _hostops.cg_direction(step, r, p, part, state)
            ac.check_direction(step, after, ac.snapshot(r=r, p=p, part=part, state=state))
            assert all(bool(torch.isfinite(t).all()) for t in (p, v, r, part)) and bool(torch.isfinite(state[[0, 1, 2, 3, 4, 5, 6, 7]]).all())


def test_host_cg_solve_is_cg():
    dt = torch.float64
    Phi, A1, Psi, f, x0, _ = ac.local_problem(dt)
    s1, s2 = torch.zeros(2, dtype=dt), torch.zeros(2, dtype=dt)
    a = _hostops.cg_solve(Phi, A1, Psi, f, x0, 1e-10, 10, s1)
    b = ttsolve._cg(_hostops, Phi, A1, Psi, f, x0, 1e-10, 10, s2)
    assert torch.equal(a, b) and torch.equal(s1, s2) and float(s1[0]) > 0


# ------------------------------------------------------------------ the C ABI's refusals
INVALID, UNSUPPORTED, WORKSPACE = _hip.E_INVALID, _hip.E_UNSUPPORTED, _hip.E_WORKSPACE
_BUF = [(ctypes.c_double * 64)() for _ in range(6)]
P, BP, X, R, PART, STATE = (ctypes.addressof(b) for b in _BUF)


def _dot(dtype=0, n=8, p=P, Bp=BP, part=PART, wsb=16):
    return ("ttr_cg_dot", (dtype, n, p, Bp, part, wsb, None))


def _upd(dtype=0, step=0, n=8, p=P, Bp=BP, v=X, r=R, part=PART, wsb=16, state=STATE):
    return ("ttr_cg_update", (dtype, step, n, p, Bp, v, r, part, wsb, state, None))


def _dir(dtype=0, step=0, n=8, r=R, p=P, part=PART, wsb=16, state=STATE):
    return ("ttr_cg_direction", (dtype, step, n, r, p, part, wsb, state, None))


REFUSALS = [(f(dtype=7), INVALID, "bad dtype 7") for f in (_dot, _upd, _dir)]
REFUSALS += [(f(n=0), INVALID, "n = 0 < 1") for f in (_dot, _upd, _dir)]
REFUSALS += [(f(n=1 << 57), UNSUPPORTED, "vectors too long") for f in (_dot, _upd, _dir)]
REFUSALS += [(f(wsb=15), WORKSPACE, "workspace of 15 bytes, 16 needed") for f in (_dot, _upd, _dir)]
REFUSALS += [(_dot(**{k: None}), INVALID, "ttr_cg_dot: null pointer") for k in ("p", "Bp", "part")]
REFUSALS += [(_upd(**{k: None}), INVALID, "ttr_cg_update: null pointer") for k in ("p", "Bp", "v", "r", "part", "state")]
REFUSALS += [(_dir(**{k: None}), INVALID, "ttr_cg_direction: null pointer") for k in ("r", "p", "part", "state")]
REFUSALS += [(_upd(v=P), INVALID, "the vectors overlap"), (_upd(r=BP + 8), INVALID, "the vectors overlap"),
             (_dir(r=P + 28), INVALID, "the vectors overlap"), (_dot(Bp=P), INVALID, "the vectors overlap"),
             (_upd(step=-1), INVALID, "step = -1 < 0"), (_dir(step=-1), INVALID, "step = -1 < 0")]


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
    (name, args), status, text = REFUSALS[case]
    assert getattr(lib, name)(*args) == status
    assert text in lib.ttr_last_error().decode()


def test_cabi_parts(lib):
    """ttr_cg_parts and ttr_cg_workspace_bytes are host functions of n and the dtype: the rule of ttr_ritz_parts."""
    for code, dt in ((_hip.F32, torch.float32), (_hip.F64, torch.float64)):
        V = ac.pack(dt)
        for n in ac.kernel_sizes(dt) + [10 ** 9]:
            want = min(_hip.CG_MAX_PARTS, max(1, -(-(-(-n // V)) // 1024)))
            assert lib.ttr_cg_parts(code, n) == want == lib.ttr_ritz_parts(code, n)
            assert lib.ttr_cg_workspace_bytes(code, n) == 16 * want
        assert [lib.ttr_cg_parts(code, n) for n in ac.kernel_sizes(dt)[-3:]] == [1, 2, 3]
    assert lib.ttr_cg_parts(7, 5) == INVALID and lib.ttr_cg_parts(0, 0) == INVALID
    assert lib.ttr_cg_workspace_bytes(7, 5) == INVALID and lib.ttr_cg_workspace_bytes(1, 0) == INVALID


# ------------------------------------------------------------------ wiring
def test_wiring():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert tn.ttamen.__all__ == ["tt_amen_solve"] and tn.tt_amen_solve is tn.ttamen.tt_amen_solve
    header = open(os.path.join(root, "include", "ttround_hip.h")).read()
    above, below = header.split("#define TTR_ABI_VERSION")
    for name in ("ttr_cg_parts", "ttr_cg_workspace_bytes", "ttr_cg_dot", "ttr_cg_update", "ttr_cg_direction"):
        assert name in above and re.search(r"\b{}\s*\(".format(name), below) and name in _hip.EXPORTED_SYMBOLS
    assert _hip.CG_MAX_PARTS == _hip.RITZ_MAX_PARTS == 256
    makefile = open(os.path.join(root, "tntorch_amd", "csrc", "Makefile")).read()
    assert re.search(r"^  ttr_cg\.hip \\$", makefile, flags=re.M)
    for mod in (_hipops, _hostops):
        assert all(callable(getattr(mod, n)) for n in ("cg_parts", "cg_workspace_bytes", "cg_dot", "cg_update", "cg_direction", "cg_solve"))
    assert "## 32." in open(os.path.join(root, "DESIGN.md")).read()
    assert "tt_amen_solve" in open(os.path.join(root, "README.md")).read() and "tt_amen_solve" in tn.__doc__

"""``tn.tt_eigsh`` on CPU tensors (the host mirror of the device ops) against ``torch.linalg.eigh`` of the dense fp64 matrix of
the same (cast) cores, and the mirror of the Rayleigh-Ritz step at its edges.

Bounds: the value and the dense residual are held against 4 x the worst case measured with the mirror
(``eigs_cases.MEASURED_*``); the variational cases and the exact start have bounds that follow from the arithmetic, stated
where they are used."""
import os
import re

import pytest
import torch

import eigs_cases as ec
import tntorch_amd as tn
from tntorch_amd import _hip, _hipops, _hostops, tteigs

DTYPES = ec.DTYPES


# ------------------------------------------------------------------ the solver
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("which", ec.WHICH)
@pytest.mark.parametrize("name, ranks", ec.checked_cases())
def test_value_and_residual(name, ranks, which, dt):
    """Full ranks on every matrix, and rank 1 where the extreme eigenvector has rank 1: two sweeps, the value within the measured
    bound of the dense eigenvalue, the dense residual within the measured bound and within tol."""
    A = ec.matrix(name, dt)
    torch.manual_seed(0)
    value, x, info = tn.tt_eigsh(A, ranks_tt=ranks, which=which, tol=ec.TOL[dt], return_info=True)
    err, res = ec.value_error(name, dt, which, value), ec.dense_residual(name, dt, value, x)
    print("{} ranks {} {} {}: {} sweeps, value error {:.3e}, dense residual {:.3e}".format(name, ranks, which, dt, info["sweeps"], err, res))
    assert info["converged"] and info["sweeps"] == 2 and len(info["local_residuals"]) == 2 == len(info["values"])
    assert info["local_residuals"][1] <= ec.tol_of(dt) < info["local_residuals"][0]
    assert err <= ec.value_bound(dt)
    assert res <= ec.residual_bound(dt) and res <= ec.tol_of(dt)
    assert abs(info["residual"] - res) <= 0.05 * res + 64 * ec.unit(dt)
    assert info["values"][-1] == float(value.double()) or abs(info["values"][-1] - float(value)) <= ec.eps(dt) * abs(float(value))
    assert value.dim() == 0 and value.dtype == dt and all(c.dtype == dt and not c.requires_grad for c in x.cores)
    dims = ec.MATRICES[name][1]
    want = ranks if hasattr(ranks, "__len__") else [ranks] * (len(dims) - 1)
    assert [int(r) for r in x.ranks_tt] == [1] + list(want) + [1]
    assert abs(float(ec.dense(x).norm()) - 1.0) <= 16 * len(dims) * ec.eps(dt)


@pytest.mark.parametrize("name", ec.RANK_ONE)
def test_rank_one_cases_have_rank_one_eigenvectors(name):
    """What makes ranks_tt=1 exact on these matrices: every unfolding of both extreme eigenvectors has one singular value."""
    _, dims, _, _, V = ec.case(name, torch.float64)
    for v in (V[:, 0], V[:, -1]):
        for k in range(1, len(dims)):
            s = torch.linalg.svdvals(v.reshape(int(torch.tensor(dims[:k]).prod()), -1))
            assert float(s[1]) <= 1e-12 * float(s[0]), (name, k)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("which", ec.WHICH)
@pytest.mark.parametrize("name", ec.RANK_TWO)
def test_rank_two_is_variational(name, which, dt):
    """Rank 2 is below the eigenvector's rank: the value is a Rayleigh quotient, so it lies inside the spectrum, and a sweep
    never moves it the wrong way.  Both hold up to the rounding of the value, 32 eps |value|."""
    A = ec.matrix(name, dt)
    l, _ = ec.truth(name, dt, which)
    x0 = ec.start(name, dt, 2, seed=3)
    sign = 1.0 if which == "SA" else -1.0
    values = []
    for nswp in (1, 2, 3):
        value, x = tn.tt_eigsh(A, x0=x0, which=which, nswp=nswp, tol=ec.TOL[dt])
        values.append(float(value))
        # the value is the Rayleigh quotient of the train returned
        xd = ec.dense(x)
        rq = float(xd @ (ec.case(name, dt)[2] @ xd) / (xd @ xd))
        assert abs(rq - values[-1]) <= 32 * ec.eps(dt) * abs(rq)
    print("rank 2 {} {} {}: values {} against {}".format(name, which, dt, values, l))
    for v in values:
        assert sign * (v - l) >= -32 * ec.eps(dt) * abs(l)
    for before, after in zip(values, values[1:]):
        assert sign * (after - before) <= 32 * ec.eps(dt) * abs(before)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("which", ec.WHICH)
def test_exact_start_is_left_alone(which, dt):
    """x0 = the exact (rank-1) eigenvector of laplace: the first residual of every site is below tol, so one sweep converges, every
    local solve is frozen at its first step, and x is x0 / ||x0|| up to the QR steps' rounding, 16 N eps."""
    name = "laplace"
    G, dims, D, w, V = ec.case(name, dt)
    # the eigenvectors of shift I + c sum L_k are Kronecker products of those of L = tridiag(-1, 2, -1)
    cores = []
    for n in dims:
        lw, lv = torch.linalg.eigh(ec.lap(n))
        cores.append((lv[:, 0] if which == "SA" else lv[:, -1]).to(dt)[None, :, None])
    x0 = tn.Tensor([3.0 * cores[0]] + cores[1:])
    keep = [c.clone() for c in x0.cores]
    calls = []
    orig = _hostops.ritz_update

    def spy(mode, which_, first, rel, part, X, AX, W, AW, P, AP, state, sweep):
        orig(mode, which_, first, rel, part, X, AX, W, AW, P, AP, state, sweep)
        calls.append((mode, state.clone()))

    _hostops.ritz_update = spy
    try:
        value, x, info = tn.tt_eigsh(ec.matrix(name, dt), x0=x0, which=which, tol=ec.TOL[dt], local_iters=3, return_info=True)
    finally:
        _hostops.ritz_update = orig
    assert info["sweeps"] == 1 and info["converged"]
    steps = [s for m, s in calls if m == _hostops.RITZ_STEP]
    assert len(steps) == 3 * (2 * len(dims) - 2) and all(float(s[2]) == 1.0 and float(s[3]) == 0.0 for s in steps)
    assert all(torch.equal(a, b) for a, b in zip(keep, x0.cores))
    xd, x0d = ec.dense(x), ec.dense(x0)
    x0d = x0d / x0d.norm()
    assert float((xd - x0d).abs().max()) <= 16 * len(dims) * ec.eps(dt)
    assert ec.value_error(name, dt, which, value) <= ec.value_bound(dt)


def test_bookkeeping(capsys):
    dt = torch.float64
    A = ec.matrix("laplace", dt)
    assert tn.tteigs.__all__ == ["tt_eigsh"] and tn.tt_eigsh is tn.tteigs.tt_eigsh and tn.ttsolve.__all__ == ["tt_solve"]
    before = dict(tteigs.READBACKS)
    x0 = ec.start("laplace", dt, 2, seed=1)
    keep = [c.clone() for c in x0.cores]
    value, x, info = tn.tt_eigsh(A, x0=x0, tol=1e-9, verbose=True, return_info=True)
    assert sorted(info) == ["converged", "local_residuals", "residual", "sweeps", "values"]
    assert tteigs.READBACKS["sweep"] - before["sweep"] == info["sweeps"] and tteigs.READBACKS["residual"] - before["residual"] == 1
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("tt_eigsh: sweep")]
    assert len(lines) == info["sweeps"] == len(info["local_residuals"]) == len(info["values"])
    assert all(isinstance(v, float) for v in info["local_residuals"] + info["values"]) and isinstance(info["residual"], float)
    assert all(torch.equal(a, b) for a, b in zip(keep, x0.cores))
    assert [int(r) for r in x.ranks_tt] == [int(r) for r in x0.ranks_tt]
    before = dict(tteigs.READBACKS)
    out = tn.tt_eigsh(A, x0=x0, nswp=1)
    assert len(out) == 2 and tteigs.READBACKS["sweep"] - before["sweep"] == 1 and tteigs.READBACKS["residual"] == before["residual"]
    # orthonormal cores up to the last visited site (site 1: cores 2.. are right-orthonormal), the norm in core 0
    for c in out[1].cores[1:]:
        m = c.reshape(c.shape[0], -1)
        assert float((m @ m.t() - torch.eye(m.shape[0], dtype=dt)).abs().max()) <= 64 * ec.eps(dt)
    assert abs(float(out[1].cores[0].norm()) - 1.0) <= 64 * ec.eps(dt)
    # grad operands on the CPU: the call runs under no_grad and returns detached cores
    for c in A.cores:
        c.requires_grad_(True)
    value, y = tn.tt_eigsh(A, ranks_tt=1, tol=1e-9)
    assert not value.requires_grad and all(not c.requires_grad and c.grad_fn is None for c in y.cores)


def test_wiring():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "ttround_hip.h")).read()
    above, below = header.split("#define TTR_ABI_VERSION")
    assert _hip.ABI_VERSION == 17
    for name in ("ttr_ritz_parts", "ttr_ritz_workspace_bytes", "ttr_ritz_gram", "ttr_ritz_update"):
        assert name in above and re.search(r"\b{}\s*\(".format(name), below) and name in _hip.EXPORTED_SYMBOLS
    assert (_hip.RITZ_INIT, _hip.RITZ_STEP, _hip.RITZ_SA, _hip.RITZ_LA) == (
        _hostops.RITZ_INIT, _hostops.RITZ_STEP, _hostops.RITZ_SA, _hostops.RITZ_LA)
    assert _hip.RITZ_DROP == _hostops.RITZ_DROP == 64 and _hip.RITZ_MAX_PARTS == 256
    makefile = open(os.path.join(root, "tntorch_amd", "csrc", "Makefile")).read()
    assert re.search(r"^  ttr_ritz\.hip \\$", makefile, flags=re.M)
    for mod in (_hipops, _hostops):
        assert all(callable(getattr(mod, n)) for n in ("ritz_parts", "ritz_workspace_bytes", "ritz_gram", "ritz_update"))
    assert "## 30." in open(os.path.join(root, "DESIGN.md")).read()
    assert "tt_eigsh" in open(os.path.join(root, "README.md")).read() and "tt_eigsh" in tn.__doc__


def test_refusals():
    dt = torch.float64
    A = ec.matrix("laplace", dt)
    dims = ec.MATRICES["laplace"][1]
    b = ec.start("laplace", dt, 2)
    ok = dict(ranks_tt=2)
    with pytest.raises(ValueError, match="must be a TTMatrix"):
        tn.tt_eigsh(b, **ok)
    with pytest.raises(ValueError, match="x0 must be a tntorch_amd.Tensor"):
        tn.tt_eigsh(A, x0=b.torch())
    with pytest.raises(ValueError, match="batched"):
        tn.tt_eigsh(tn.TTMatrix([c[None] for c in A.cores], None, dims, dims), **ok)
    with pytest.raises(ValueError, match="batched"):
        tn.tt_eigsh(A, x0=tn.Tensor([c[None] for c in b.cores], batch=True))
    with pytest.raises(ValueError, match="boundary ranks"):
        tn.tt_eigsh(tn.TTMatrix([torch.cat([A.cores[0]] * 2, dim=0)] + A.cores[1:], None, dims, dims), **ok)
    with pytest.raises(ValueError, match="boundary ranks of x0"):
        tn.tt_eigsh(A, x0=tn.Tensor([torch.cat([b.cores[0]] * 2, dim=0)] + b.cores[1:]))
    with pytest.raises(ValueError, match="3 modes, x0 has 2"):
        tn.tt_eigsh(A, x0=tn.Tensor([b.cores[0], b.cores[1][:, :, :1]]))
    wide = [A.cores[0], A.cores[1][:, :, :2], A.cores[2]]
    with pytest.raises(ValueError, match="mode 1 of the matrix is not square"):
        tn.tt_eigsh(tn.TTMatrix(wide, None, dims, [4, 2, 5]), **ok)
    with pytest.raises(ValueError, match="mode 0 of x0 has size 3"):
        tn.tt_eigsh(A, x0=tn.Tensor([b.cores[0][:, :3], b.cores[1], b.cores[2]]))
    with pytest.raises(ValueError, match="float32 or float64"):
        tn.tt_eigsh(tn.TTMatrix([c.half() for c in A.cores], None, dims, dims), **ok)
    with pytest.raises(ValueError, match="same dtype"):
        tn.tt_eigsh(A, x0=tn.Tensor([c.float() for c in b.cores]))
    with pytest.raises(ValueError, match="tt_eigsh: the operands must be on the same device"):
        tn.tt_eigsh(A, x0=tn.Tensor([c.to("meta") for c in b.cores]))
    with pytest.raises(ValueError, match="x0 or ranks_tt"):
        tn.tt_eigsh(A)
    with pytest.raises(ValueError, match="ranks_tt needs 2 entries"):
        tn.tt_eigsh(A, ranks_tt=[2])
    for bad in (dict(nswp=0), dict(local_iters=0), dict(tol=0.0), dict(tol=-1e-3)):
        with pytest.raises(ValueError, match="nswp and local_iters|tol must be positive"):
            tn.tt_eigsh(A, **ok, **bad)
    for bad in ("SM", "sa", None):
        with pytest.raises(ValueError, match="which must be 'SA' or 'LA'"):
            tn.tt_eigsh(A, which=bad, **ok)
    with pytest.raises(NotImplementedError, match="CP cores"):
        tn.tt_eigsh(A, x0=tn.Tensor([torch.rand(n, 2, dtype=dt) for n in dims]))
    before = dict(tteigs.READBACKS)
    with pytest.raises(ValueError, match="zero train"):
        tn.tt_eigsh(A, x0=tn.Tensor([torch.zeros_like(c) for c in b.cores]))
    assert tteigs.READBACKS["sweep"] - before["sweep"] == 1          # raised after that sweep's readback
    bad = [c.clone() for c in A.cores]
    bad[1][0, 1, 1, 0] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        tn.tt_eigsh(tn.TTMatrix(bad, None, dims, dims), x0=b)


# ------------------------------------------------------------------ the mirror of the step
def _fresh(dt):
    return torch.zeros(8, dtype=torch.float64), torch.zeros(4, dtype=torch.float64)


def _step(vs, which=_hostops.RITZ_SA, rel=0.0, first=1, p=True, state=None, sweep=None):
    X, AX, W, AW, P, AP = vs
    st, sw = _fresh(X.dtype)
    state = st if state is None else state
    sweep = sw if sweep is None else sweep
    part = _hostops.ritz_gram(_hostops.RITZ_STEP, X, AX, W, AW, P if p else None, AP if p else None)
    _hostops.ritz_update(_hostops.RITZ_STEP, which, first, rel, part, X, AX, W, AW, P if p else None, AP if p else None, state, sweep)
    return state, sweep


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("which", [_hostops.RITZ_SA, _hostops.RITZ_LA])
def test_mirror_step(which, dt):
    """A generic step: the new X has norm 1, c0 >= 0, theta' is the Rayleigh quotient of the new pair and not worse than theta."""
    n = 257
    vs = [v.clone() for v in ec.ritz_vectors(n, dt, seed=1)]
    X, AX = vs[0].double(), vs[1].double()
    theta = float(X @ AX / (X @ X))
    state, sweep = _step(vs, which=which)
    Xn, AXn, Wn = vs[0].double(), vs[1].double(), vs[2].double()
    assert float(state[3]) == 0 and float(state[2]) == 0 and float(state[7]) == 3 and float(state[4]) >= 0
    assert abs(float(Xn.norm()) - 1.0) <= 8 * ec.eps(dt)
    assert abs(float(Xn @ AXn) - float(state[0])) <= 8 * ec.eps(dt) * float(AXn.norm())
    sign = 1.0 if which == _hostops.RITZ_SA else -1.0
    assert sign * (float(state[0]) - theta) <= 8 * ec.eps(dt) * abs(theta)
    assert float((Wn - (AXn - float(state[0]) * Xn)).abs().max()) <= 4 * ec.eps(dt) * float(AXn.abs().max())
    assert float(sweep[0]) == float(state[1]) > 0 and float(sweep[1]) == 0 and float(sweep[2]) == float(state[0])


@pytest.mark.parametrize("dt", DTYPES)
def test_mirror_edges(dt):
    n = 64
    base = ec.ritz_vectors(n, dt, seed=2)
    # P = None: two directions
    vs = [v.clone() for v in base]
    state, _ = _step(vs, p=False)
    assert float(state[7]) == 2 and float(state[6]) == 0 and all(bool(torch.isfinite(v).all()) for v in vs)
    assert torch.equal(vs[4], base[4]) and torch.equal(vs[5], base[5])           # P, AP neither read nor written
    # W = 0: an exact eigenvector, frozen whatever rel is
    vs = [v.clone() for v in base]
    vs[2].zero_(), vs[3].zero_()
    keep = [v.clone() for v in vs]
    state, _ = _step(vs, rel=0.0)
    assert float(state[2]) == 1 and float(state[1]) == 0 and float(state[7]) == 0 and all(torch.equal(a, b) for a, b in zip(keep, vs))
    # W parallel to P: the pair spans one direction, one is dropped
    vs = [v.clone() for v in base]
    vs[4].copy_(2 * vs[2]), vs[5].copy_(2 * vs[3])
    state, _ = _step(vs)
    assert float(state[7]) == 2 and float(state[3]) == 0 and all(bool(torch.isfinite(v).all()) for v in vs)
    assert abs(float(vs[0].double().norm()) - 1.0) <= 8 * ec.eps(dt)
    # frozen: rel above res, nothing written
    vs = [v.clone() for v in base]
    keep = [v.clone() for v in vs]
    state, sweep = _step(vs, rel=2.0)
    assert float(state[2]) == 1 and 0 < float(state[1]) <= 1 and all(torch.equal(a, b) for a, b in zip(keep, vs))
    assert float(sweep[0]) == float(state[1])
    # a non-finite sum: flag 1, nothing written, counted
    vs = [v.clone() for v in base]
    vs[2][5] = float("inf")
    keep = [v.clone() for v in vs]
    state, sweep = _step(vs)
    assert float(state[3]) == 1 and float(sweep[1]) == 1 and float(sweep[3]) == 1
    assert all(torch.equal(a, b) for a, b in zip(keep, vs))
    # X = 0 in INIT: flag 2
    vs = [v.clone() for v in base]
    vs[0].zero_(), vs[1].zero_()
    keep = [v.clone() for v in vs]
    state, sweep = _fresh(dt)
    part = _hostops.ritz_gram(_hostops.RITZ_INIT, vs[0], vs[1])
    _hostops.ritz_update(_hostops.RITZ_INIT, _hostops.RITZ_SA, 0, 0.0, part, vs[0], vs[1], vs[2], None, vs[4], vs[5], state, sweep)
    assert float(state[3]) == 2 and float(sweep[1]) == 1 and float(sweep[3]) == 2 and all(torch.equal(a, b) for a, b in zip(keep, vs))
    assert float(state[7]) == 0 and float(state[0]) == 0 and state[4:7].tolist() == [1.0, 0.0, 0.0]     # no direction kept
    # a non-finite sum in INIT: flag 1, kept 0 as well
    vs = [v.clone() for v in base]
    vs[1][2] = float("nan")
    keep = [v.clone() for v in vs]
    state, sweep = _fresh(dt)
    part = _hostops.ritz_gram(_hostops.RITZ_INIT, vs[0], vs[1])
    _hostops.ritz_update(_hostops.RITZ_INIT, _hostops.RITZ_SA, 0, 0.0, part, vs[0], vs[1], vs[2], None, vs[4], vs[5], state, sweep)
    assert float(state[3]) == 1 and float(state[7]) == 0 and float(sweep[1]) == 1
    assert all(torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)) for a, b in zip(keep, vs))            # nothing written
    # INIT on a good X: normalised, W the residual, P = AP = 0
    vs = [v.clone() for v in base]
    state, sweep = _fresh(dt)
    part = _hostops.ritz_gram(_hostops.RITZ_INIT, vs[0], vs[1])
    assert float(part[0, 1:6].abs().max()) == 0 and float(part[0, 7:].abs().max()) == 0
    _hostops.ritz_update(_hostops.RITZ_INIT, _hostops.RITZ_SA, 0, 0.0, part, vs[0], vs[1], vs[2], None, vs[4], vs[5], state, sweep)
    assert abs(float(vs[0].double().norm()) - 1.0) <= 8 * ec.eps(dt) and float(vs[4].abs().max()) == 0 == float(vs[5].abs().max())
    assert float(sweep[0]) == 0 and float(sweep[2]) == float(state[0]) and float(state[7]) == 1


def test_mirror_far_past_convergence():
    """The 7 x 7 one-mode problem run far past convergence with rel = 0: the directions degenerate into rounding noise, the
    dropping rule keeps the pencil regular, nothing turns non-finite and the value stays."""
    for dt in DTYPES:
        A = ec.matrix("one", dt)
        value, x, info = tn.tt_eigsh(A, ranks_tt=[], tol=1e-300, nswp=2, local_iters=200, return_info=True)
        assert ec.value_error("one", dt, "SA", value) <= ec.value_bound(dt)
        assert all(bool(torch.isfinite(c).all()) for c in x.cores)

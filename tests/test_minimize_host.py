"""tn.minimum / tn.argmin / tn.maximum / tn.argmax on CPU tensors against the dense optimum and against
tests/golden/minimize_f64.npz (recorded from the unmodified reference by tools/gen_minimize_golden.py), the keyword contract of
``cross(..., _minimize=True)``, and the host mirror of ttr_minimize_step on the edge list of tests/test_minimize_kernels_gpu.py.

What "the value is the sample itself" is checked against.  ``minimum`` returns a sample evaluated from the train's cores (left
interface x core x right interface), bit for bit.  Where the train holds the dense entries exactly (quad8, quad5764: the
identity-padded full-rank train multiplies them by 0 and 1 only) that sample IS ``dense[argmin]`` and equality with it is asserted.
The sinquad train is a TT-SVD at ranks_tt=8 (measured: max |train - dense| = 5.0e-14) and randn3 is evaluated by ``t.torch()`` in
another order of the products than a fibre (measured: 1 ulp apart at the minimiser), so there the value cannot equal the dense
entry bit for bit.  For every case, those two included, the value is asserted to equal, exactly, the smallest of all the values the
function returned during the call; against the dense entry the two get the bound of ``minimize_cases.value_bound`` plus the
train's own distance from the dense tensor."""
import math
import os
import re

import numpy as np
import pytest
import torch

import minimize_cases as mc
import tntorch_amd as tn
from tntorch_amd import _hip, _hostops

ROOT = mc.ROOT
_BUILT = {}


def case(name):
    if name not in _BUILT:
        _BUILT[name] = mc.build(name, tn)
    return _BUILT[name]


@pytest.fixture
def f64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


def optimum(d, fn):
    return d.min() if fn in ("minimum", "argmin") else d.max()


def test_fixture_and_trains():
    z = mc.fixture()
    t, d = case("randn3")
    for n, c in enumerate(t.cores):   # the same random train as the reference drew
        np.testing.assert_array_equal(c.numpy(), z["randn3_core{}".format(n)])
    for name in mc.CASES:
        t, d = case(name)
        assert d.dtype == torch.float64 and t.cores[0].dtype == torch.float64
        assert float(d.min()) == float(z[name + "_dense_min"]) and float(d.max()) == float(z[name + "_dense_max"])
        if name in mc.EXACT_TRAIN:
            assert torch.equal(t.torch(), d)
        for lo in (True, False):   # how many optimisers the dense tensor has
            n = int((d == (d.min() if lo else d.max())).sum())
            assert (n == 1) if name in mc.UNIQUE else (n >= 1), (name, lo, n)
    d = case("sinquad")[1]
    assert int((d == d.min()).sum()) > 1 or int((d == d.max()).sum()) > 1   # exactly tied optimisers


@pytest.mark.parametrize("fn", mc.FUNCTIONS)
@pytest.mark.parametrize("s", mc.SEEDS)
@pytest.mark.parametrize("name", mc.CASES)
def test_against_dense_and_reference(name, s, fn, f64):
    z = mc.fixture()
    t, d = case(name)
    ref = z["{}_s{}_{}".format(name, s, fn)]
    sign = 1.0 if fn in ("minimum", "argmin") else -1.0
    seen = []

    def spy(x):
        seen.append(x.detach().clone())
        return x

    mc.seed(s)
    r = getattr(tn, fn)(t, function=spy)
    mc.seed(s)
    _, info = tn.cross(tensors=t, function=lambda x: sign * x, rmax=10, max_iter=10, verbose=False, return_info=True, _minimize=True)
    assert info["nsamples"] == int(z["{}_s{}_nsamples".format(name, s)])
    pos, val = info["argmin"], sign * info["min"]
    assert float(d[pos]) == float(optimum(d, fn))                                  # the dense optimum was found ...
    if name in mc.UNIQUE:
        assert pos == tuple(int(x) for x in torch.nonzero(d == optimum(d, fn))[0])  # ... at the dense optimiser
    samples = torch.cat(seen[1:])                                                  # (the first call evaluates the validation set)
    assert info["nsamples"] == samples.numel()
    assert float(val) == float(optimum(samples, fn))                               # the value is the evaluated sample itself
    if name in mc.EXACT_TRAIN:
        assert float(val) == float(d[pos])
    else:
        assert abs(float(val) - float(d[pos])) <= float((t.torch() - d).abs().max()) + mc.value_bound(t, pos)
    if fn.startswith("arg"):
        assert r == pos and isinstance(r, tuple) and len(r) == t.dim() and all(type(x) is int for x in r)
        if name in mc.UNIQUE:
            assert r == tuple(int(x) for x in ref)
    else:
        assert isinstance(r, torch.Tensor) and r.dim() == 0 and r.dtype == torch.float64 and r.device.type == "cpu"
        assert float(r) == float(val)
        print("{} s{} {}: ours {!r}, reference {!r}, relative deviation {:.3e}".format(
            name, s, fn, float(r), float(ref), abs(float(r) - float(ref)) / abs(float(r))))
        assert abs(float(r) - float(ref)) <= mc.REF_RTOL * abs(float(r))


def test_function_of_two_tensors(f64):
    ta, da = case("quad5764")
    g = torch.Generator().manual_seed(3)
    db = torch.rand(5, 7, 6, 4, generator=g, dtype=torch.float64) - 0.4
    tb = tn.Tensor(db)
    prod = da * db
    f = lambda a, b: a * b
    mc.seed(0)
    lo = tn.minimum([ta, tb], function=f)
    mc.seed(0)
    plo = tn.argmin([ta, tb], function=f)
    mc.seed(0)
    hi = tn.maximum([ta, tb], function=f)
    mc.seed(0)
    phi = tn.argmax([ta, tb], function=f)
    assert float(lo) == float(prod.min()) == float(prod[plo]) and float(hi) == float(prod.max()) == float(prod[phi])


def test_domain_and_matrix_argument(f64):
    domain = [torch.linspace(-1, 1, 9), torch.linspace(0, 2, 7), torch.linspace(-2, 1, 8)]
    c = torch.tensor([0.3, 1.4, -0.9])
    f = lambda X: ((X - c) ** 2).sum(dim=1) + 0.25
    grids = torch.meshgrid(*domain, indexing="ij")
    d = f(torch.stack([g.reshape(-1) for g in grids], dim=1)).reshape(9, 7, 8)
    mc.seed(1)
    v = tn.minimum(function=f, domain=domain, function_arg="matrix")
    mc.seed(1)
    p = tn.argmin(function=f, domain=domain, function_arg="matrix")
    assert p == tuple(int(x) for x in torch.nonzero(d == d.min())[0])
    # (the rows of the matrix are the grid values themselves: a rank-1 train of ones and one vector holds them exactly)
    assert float(v) == float(d[p]) == float(d.min())
    mc.seed(1)
    assert tn.argmax(function=f, domain=domain, function_arg="matrix") == tuple(int(x) for x in torch.nonzero(d == d.max())[0])


def test_minimum_exactly_zero(f64):
    d = mc.dense("quad8_zero")
    assert float(d.min()) == 0.0 and float(d[2, 5, 0, 7]) == 0.0 and int((d == 0).sum()) == 1
    t = tn.Tensor(d)
    for s in mc.SEEDS:
        mc.seed(s)
        v = tn.minimum(t)
        mc.seed(s)
        assert float(v) == 0.0 and tn.argmin(t) == (2, 5, 0, 7)


def test_cross_without_minimize_is_unchanged(f64):
    """_minimize=False is the default path: the golden of tn.cross replays (index sets, sample count and generator state exact, as
    tests/test_cross_host.py asserts without the keyword), and an explicit False chooses the same index sets as the default.
    (The cores of two IDENTICAL host calls already differ in the last bits, measured up to 1e-15 here: LAPACK's lstsq and
    einsum are not run-to-run reproducible; so the cores are compared to 1e-12.)"""
    from test_cross_host import replay_cross

    assert sum(1 for _ in replay_cross("cpu", 1e-10)) == 5
    domain = [torch.linspace(0, 1, 8)] * 3
    f = lambda x, y, z: 1 / (1 + x + 2 * y + 3 * z)
    out = []
    for kw in ({}, {"_minimize": False}):
        mc.seed(4)
        out.append(tn.cross(f, domain=domain, max_iter=3, verbose=False, return_info=True, suppress_warnings=True, **kw))
    (ta, ia), (tb, ib) = out
    assert all(a.shape == b.shape and float((a - b).abs().max()) <= 1e-12 * float(a.abs().max()) for a, b in zip(ta.cores, tb.cores))
    assert all(np.array_equal(a, b) for k in ("lsets", "rsets", "left_locals") for a, b in zip(ia[k], ib[k]))
    assert ia["min"] == 0 and ia["argmin"] is None and ia["nsamples"] == ib["nsamples"]


def test_errors_and_printout(f64, capsys, caplog):
    with pytest.raises(ValueError, match="Batched"):
        tn.minimum(tn.rand([4] * 3, ranks_tt=2, batch=True))
    t, _ = case("quad8")
    for fn in (tn.minimum, tn.argmax):
        with pytest.raises(ValueError, match="Invalid return value"):
            fn(t, function=lambda x: torch.where(x > 3, x * float("nan"), x))
    with pytest.raises(ValueError, match="Invalid return value"):
        tn.minimum(t, function=lambda x: torch.where(x > 3, x * float("inf"), x))
    capsys.readouterr()
    with caplog.at_level("WARNING"):
        mc.seed(0)
        tn.minimum(t, max_iter=2, verbose=True)
    out = capsys.readouterr().out
    assert len(re.findall(r"\| best: 0\.68 \|", out)) == 2 and "| eps:" not in out
    assert not caplog.records   # the "larger than eps" warning is suppressed


def test_exports_and_docs():
    for name in mc.FUNCTIONS:
        assert name in tn.cross.__globals__["__all__"] and callable(getattr(tn, name))
    doc = tn.cross.__globals__["__doc__"]
    scope = [p for p in doc.split("\n\n") if "out of scope" in p]   # the paragraph that says what is left out
    assert len(scope) == 1 and "cross_forward" in scope[0] and "minimum" not in scope[0] and "argm" not in scope[0]
    header = open(os.path.join(ROOT, "include", "ttround_hip.h")).read()
    for name in ("ttr_minimize_step", "ttr_minimize_workspace_bytes"):
        assert re.search(r"\b{}\s*\(".format(name), header) and name in _hip.EXPORTED_SYMBOLS
    assert _hip.ABI_VERSION == 17 and _hip.MINIMIZE_BLOCK_ELEMS == 4096
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert re.search(r"^## 22\.", design, flags=re.M) and "ttr_minimize_step" in design and "tn.minimum" in readme
    assert "gen_minimize_golden.py" in open(os.path.join(ROOT, "tools", "README.md")).read()


# ------------------------------------------------------------------------------------------------ the mirror of the step
E = _hip.MINIMIZE_BLOCK_ELEMS


def state(dtype, N, best=None, sentinel=-7):
    return (torch.tensor([0.0 if best is None else best], dtype=dtype), torch.full((N,), sentinel, dtype=torch.int64),
            torch.tensor([0 if best is None else 1, 0], dtype=torch.int32))


def sets(Ra, Rb, nl, nr):
    """Index sets with distinct entries everywhere: row a of lset is 1000 a + column, row c of rset 100000 + 1000 c + column."""
    lset = 1000 * torch.arange(Ra)[:, None] + torch.arange(nl + 1)[None, :]
    rset = 100000 + 1000 * torch.arange(Rb)[:, None] + torch.arange(nr + 1)[None, :]
    return lset, rset


def expected_pos(m, Ra, I, Rb, lset, rset):
    a, i, c = m // (I * Rb), (m // Rb) % I, m % Rb
    return lset[a, 1:].tolist() + [i] + rset[c, :-1].tolist()


def values(M, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(M, generator=g, dtype=torch.float64) * 8 + 1).to(dtype)   # in [1, 9): distinct from the planted minima


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("M", [1, 3, 63, 64, 65, E - 1, E, E + 1, 3 * E + 5])
def test_mirror_sizes_shapes_and_locations(M, dtype):
    spots = sorted({0, M - 1, min(E, M - 1), max(M - 2, 0)})
    for Ra, I, Rb in ((1, M, 1), (M, 1, 1), (1, 1, M)):
        lset, rset = sets(Ra, Rb, 2, 1)
        for m in spots:
            e = values(M, dtype, M)
            e[m] = 0.5
            orig = e.clone()
            best, pos, flags = state(dtype, 4)
            out = _hostops.minimize_step(e, Ra, I, Rb, lset, rset, best, pos, flags)
            assert out is e and torch.equal(e, math.pi / 2 - torch.atan(orig))     # m0 = 0 while nothing is found
            assert float(best) == 0.5 and flags.tolist() == [1, 0] and pos.tolist() == expected_pos(m, Ra, I, Rb, lset, rset)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_mirror_3d_positions_and_strides(dtype):
    Ra, I, Rb = 3, 5, 7
    for nl, nr in ((0, 4), (4, 0), (2, 2), (0, 0)):
        lset, rset = sets(Ra, Rb, nl, nr)
        wide_l, wide_r = torch.full((Ra, nl + 4), -1), torch.full((Rb, nr + 3), -1)
        wide_l[:, : nl + 1], wide_r[:, : nr + 1] = lset, rset
        for m in (0, 52, 104):
            for L, R in ((lset, rset), (wide_l[:, : nl + 1], wide_r[:, : nr + 1])):
                e = values(Ra * I * Rb, dtype, 1)
                e[m] = -2.0
                best, pos, flags = state(dtype, nl + 1 + nr)
                _hostops.minimize_step(e, Ra, I, Rb, L, R, best, pos, flags)
                assert pos.tolist() == expected_pos(m, Ra, I, Rb, lset, rset) and float(best) == -2.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_mirror_ties_state_and_nonfinite(dtype):
    M = 2 * E + 9
    lset, rset = sets(1, 1, 1, 1)
    run = lambda e, st: _hostops.minimize_step(e, 1, M, 1, lset, rset, *st)
    for a, b in ((5, E + 17), (5, 40), (M - 3, M - 1)):           # equal minima: the lower index wins
        e = values(M, dtype)
        e[a] = e[b] = 0.25
        st = state(dtype, 3)
        run(e, st)
        assert st[1].tolist() == [1, a, 100000]
    for first, second in ((-0.0, 0.0), (0.0, -0.0)):              # -0.0 == +0.0: the first of them, with its sign
        e = values(M, dtype)
        e[7], e[E + 3] = first, second
        st = state(dtype, 3)
        run(e, st)
        assert st[1][1] == 7 and math.copysign(1.0, float(st[0])) == math.copysign(1.0, first)
    e = values(M, dtype)
    st = state(dtype, 3)
    run(e.clone(), st)                                            # an empty state adopts a positive minimum
    lo, at = float(e.min()), int(e.argmin())
    assert lo > 0 and float(st[0]) == lo and st[1][1] == at and st[2].tolist() == [1, 0]
    for cand, wins in ((lo, False), (lo - 0.5, True), (lo + 0.5, False)):   # equal: untouched; smaller: both; larger: neither
        e2 = values(M, dtype, 5) + 8
        e2[11] = cand
        st2 = state(dtype, 3, best=lo)
        o2 = e2.clone()
        run(e2, st2)
        assert torch.equal(e2, math.pi / 2 - torch.atan(o2 - torch.tensor(lo, dtype=dtype)))   # m0 = the best so far
        assert (float(st2[0]), st2[1].tolist()) == ((cand, [1, 11, 100000]) if wins else (lo, [-7] * 3)) and st2[2].tolist() == [1, 0]
    for bad in ([float("nan")], [float("inf")], [-float("inf")], None):     # None: every entry NaN
        e = values(M, dtype)
        e[3] = 0.125
        if bad is None:
            e[:] = float("nan")
        else:
            e[E + 1] = bad[0]
        o = e.clone()
        for st in (state(dtype, 3), state(dtype, 3, best=4.0)):
            before = (float(st[0]), st[1].tolist(), int(st[2][0]))
            ee = e.clone()
            run(ee, st)
            assert (float(st[0]), st[1].tolist(), int(st[2][0])) == before and int(st[2][1]) == 1
            fin = torch.isfinite(o)
            want = math.pi / 2 - torch.atan(o - (4.0 if before[2] else 0.0))
            assert torch.equal(ee[fin], want[fin])                          # the finite entries are still transformed

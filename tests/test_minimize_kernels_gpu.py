"""ttr_minimize_step through the C ABI on a real MI355X, fp32 and fp64, against its mirror ``_hostops.minimize_step``: the state
(best value, position, found / invalid) bit for bit, the transformed block against ``pi/2 - atan(e - m0)`` computed by torch on
the same GPU.

Sizes, with E = TTR_MINIMIZE_BLOCK_ELEMS (one workgroup's chunk): 1, 3, 63, 64, 65, E - 1, E, E + 1, 3 E + 5, each as
(1, M, 1), (M, 1, 1) and (1, 1, M), aligned and as a view one element off an aligned base, with the minimum at 0, M - 1, the first
element of the second workgroup and in the non-vector tail; one 3-d block (3, 5, 7).

Transformed values: the largest deviation from torch's own evaluation measured over every block of this file and over
``ulp_probe`` (2^20 values from 1e-6 to 1e6 in both signs, m0 = 0 and m0 = -3.7) is ULP_MEASURED ulps of the result; the tests
assert ULP_BOUND = twice that, rounded up to a power of two."""
import math

import pytest
import torch

from tntorch_amd import _hip as h
from tntorch_amd import _hipops, _hostops

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
E = h.MINIMIZE_BLOCK_ELEMS
SIZES = [1, 3, 63, 64, 65, E - 1, E, E + 1, 3 * E + 5]
ULP_MEASURED = {torch.float32: 0.0, torch.float64: 0.0}   # measured on an MI355X (gfx950, ROCm's atanf / atan on both sides)
ULP_BOUND = {torch.float32: 1.0, torch.float64: 1.0}      # 2 x 0 rounded up to a power of two: 2^0, the smallest there is
SENTINEL = -7


def ulps(got, want, fin):
    """Largest |got - want| in units of the spacing of ``want``'s dtype at ``want``, over the entries ``fin`` (those whose input
    was finite: what a non-finite entry is transformed to is unspecified)."""
    if not bool(fin.any()):
        return 0.0
    g, w = got[fin], want[fin]
    assert bool(torch.isfinite(g).all())
    spacing = torch.nextafter(w.abs(), torch.full_like(w, math.inf)) - w.abs()
    return float(((g - w).abs() / spacing).max())


def values(M, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(M, generator=g, dtype=torch.float64) * 8 + 1).to(dtype)   # in [1, 9): distinct from the planted minima


def sets(Ra, Rb, nl, nr):
    """Distinct entries everywhere, so that a wrong row or a shifted column shows."""
    lset = 1000 * torch.arange(Ra)[:, None] + torch.arange(nl + 1)[None, :]
    rset = 100000 + 1000 * torch.arange(Rb)[:, None] + torch.arange(nr + 1)[None, :]
    return lset, rset


def state(dtype, N, best=None):
    return (torch.tensor([0.0 if best is None else best], dtype=dtype), torch.full((N,), SENTINEL, dtype=torch.int64),
            torch.tensor([0 if best is None else 1, 0], dtype=torch.int32))


def widen(s):
    """The same matrix as a column slice of a wider one on the device: a row stride above the row length."""
    wide = torch.full((s.shape[0], s.shape[1] + 3), -1, dtype=torch.int64).cuda()
    wide[:, : s.shape[1]] = s.cuda()
    return wide[:, : s.shape[1]]


def device_block(e, offset):
    """``e`` on the device, 16-byte aligned (torch's allocations are) or as a view that starts one element behind such a base."""
    if not offset:
        d = e.cuda()
        assert d.data_ptr() % 16 == 0
        return d
    base = torch.empty(e.numel() + 1, dtype=e.dtype).cuda()
    assert base.data_ptr() % 16 == 0
    d = base[1:]
    d.copy_(e)
    return d


def c_step(e, Ra, I, Rb, lset, rset, best, pos, flags):
    """One ttr_minimize_step through the C ABI on the current stream; every argument is a device tensor."""
    L = h.lib()
    code = h.dtype_code(e.dtype)
    wsb = L.ttr_minimize_workspace_bytes(code, Ra * I * Rb)
    assert wsb >= 256 and wsb % 256 == 0
    ws = torch.empty(wsb, dtype=torch.uint8).cuda()
    nl, nr = lset.shape[1] - 1, rset.shape[1] - 1
    rc = L.ttr_minimize_step(code, e.data_ptr(), Ra, I, Rb, lset.data_ptr(), lset.stride(0), nl, rset.data_ptr(), rset.stride(0), nr,
                             best.data_ptr(), pos.data_ptr(), flags.data_ptr(), ws.data_ptr(), wsb,
                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.ttr_last_error()
    torch.cuda.synchronize()   # (ws must outlive the launches)


def run(e, shape, lset, rset, st, offset=False, strided=False):
    """The step on the device and its mirror on the CPU from the same inputs: the states must agree bit for bit, the block with
    torch's formula on the GPU within ULP_BOUND.  Returns the device state on the CPU and the measured ulps."""
    Ra, I, Rb = shape
    dt = e.dtype
    ed = device_block(e, offset)
    ld, rd = (widen(lset), widen(rset)) if strided else (lset.cuda(), rset.cuda())
    sd = [x.cuda() for x in st]
    m0 = sd[0][0].clone() if int(st[2][0]) else torch.zeros((), dtype=dt).cuda()
    fin = torch.isfinite(ed)
    want = math.pi / 2 - torch.atan(ed.clone() - m0)
    c_step(ed, Ra, I, Rb, ld, rd, *sd)
    eh, sh = e.clone(), [x.clone() for x in st]
    _hostops.minimize_step(eh, Ra, I, Rb, lset, rset, *sh)
    got = [x.cpu() for x in sd]
    assert got[2].tolist() == sh[2].tolist() and got[1].tolist() == sh[1].tolist(), (shape, got, sh)
    assert got[0].view(torch.int32 if dt == torch.float32 else torch.int64).item() == \
        sh[0].view(torch.int32 if dt == torch.float32 else torch.int64).item()          # the same bits: the sign of a zero too
    u = ulps(ed, want, fin)
    assert u <= ULP_BOUND[dt], (shape, u)
    return got, u


def expected_pos(m, shape, lset, rset):
    Ra, I, Rb = shape
    a, i, c = m // (I * Rb), (m // Rb) % I, m % Rb
    return lset[a, 1:].tolist() + [i] + rset[c, :-1].tolist()


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "off1"])
@pytest.mark.parametrize("M", SIZES)
def test_sizes_shapes_and_locations(M, offset, dt):
    V = 128 // torch.finfo(dt).bits                           # elements of a 16-byte pack
    head = V - 1 if offset else 0                             # elements in front of the first aligned pack
    # first and last element, the first of the second workgroup's chunk, the last pack and the elements behind it
    spots = sorted({0, M - 1, min(head + E, M - 1), max(M - 2, 0), max(head + (M - head) // V * V - 1, 0)})
    worst = 0.0
    for shape in ((1, M, 1), (M, 1, 1), (1, 1, M)):
        lset, rset = sets(shape[0], shape[2], 2, 1)
        for m in spots:
            e = values(M, dt, M)
            e[m] = 0.5
            got, u = run(e, shape, lset, rset, state(dt, 4), offset=offset)
            worst = max(worst, u)
            assert float(got[0]) == 0.5 and got[2].tolist() == [1, 0] and got[1].tolist() == expected_pos(m, shape, lset, rset)
    print("M = {} {} {}: largest deviation {} ulp".format(M, "off1" if offset else "aligned", dt, worst))


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "fp64"])
def test_3d_block_positions_and_strides(dt):
    shape = (3, 5, 7)
    for nl, nr in ((0, 4), (4, 0), (2, 2), (0, 0)):           # j = 0, j = N - 1, N = 5 in the middle, N = 1
        lset, rset = sets(3, 7, nl, nr)
        for m in (0, 52, 104):
            for strided in (False, True):
                e = values(105, dt, 1)
                e[m] = -2.0
                got, _ = run(e, shape, lset, rset, state(dt, nl + 1 + nr), strided=strided, offset=strided)
                assert got[1].tolist() == expected_pos(m, shape, lset, rset) and float(got[0]) == -2.0
    assert expected_pos(52, shape, *sets(3, 7, 2, 2)) == [1001, 1002, 2, 103000, 103001]   # (the rule itself, written out once)


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "fp64"])
def test_ties(dt):
    M = 2 * E + 9
    lset, rset = sets(1, 1, 1, 1)
    for a, b in ((5, E + 17), (5, 40), (M - 3, M - 1), (E - 1, E)):   # two workgroups, one wave, the tail, across the chunk edge
        e = values(M, dt)
        e[a] = e[b] = 0.25
        got, _ = run(e, (1, M, 1), lset, rset, state(dt, 3))
        assert got[1].tolist() == [1, a, 100000]
    for first, second in ((-0.0, 0.0), (0.0, -0.0)):
        for a, b in ((7, E + 3), (7, 9)):
            e = values(M, dt)
            e[a], e[b] = first, second
            got, _ = run(e, (1, M, 1), lset, rset, state(dt, 3))
            assert got[1][1] == a and math.copysign(1.0, float(got[0])) == math.copysign(1.0, first)


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "fp64"])
def test_state(dt):
    M = E + 70
    lset, rset = sets(1, 1, 1, 1)
    e = values(M, dt)
    lo, at = float(e.min()), int(e.argmin())
    got, _ = run(e, (1, M, 1), lset, rset, state(dt, 3))             # an empty state adopts a positive minimum
    assert lo > 0 and float(got[0]) == lo and got[1].tolist() == [1, at, 100000] and got[2].tolist() == [1, 0]
    for cand, wins in ((lo, False), (lo - 0.5, True), (lo + 0.5, False)):
        e2 = values(M, dt, 5) + 8
        e2[E + 11] = cand
        got, _ = run(e2, (1, M, 1), lset, rset, state(dt, 3, best=lo))   # (the block is checked against m0 = lo inside)
        assert (float(got[0]), got[1].tolist()) == ((cand, [1, E + 11, 100000]) if wins else (lo, [SENTINEL] * 3))
        assert got[2].tolist() == [1, 0]


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("bad", ["nan", "inf", "-inf", "all-nan"])
def test_nonfinite(bad, dt):
    M = 2 * E + 9
    lset, rset = sets(1, 1, 1, 1)
    e = values(M, dt)
    e[3] = 0.125
    if bad == "all-nan":
        e[:] = float("nan")
    else:
        e[E + 1] = float(bad)
    for st in (state(dt, 3), state(dt, 3, best=4.0)):
        before = (float(st[0]), st[1].tolist(), int(st[2][0]))
        got, _ = run(e, (1, M, 1), lset, rset, st)                   # (run compares the finite entries' transforms)
        assert (float(got[0]), got[1].tolist(), int(got[2][0])) == before and int(got[2][1]) == 1
    st = state(dt, 3)                                                # invalid stays set; a later clean block still updates
    st[2][1] = 1
    got, _ = run(values(M, dt), (1, M, 1), lset, rset, st)
    assert got[2].tolist() == [1, 1] and got[1][1] != SENTINEL


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "fp64"])
def test_repeatable_and_wrapper(dt):
    """Two calls on the same input give the same bits in e and in the state; the package's op is the same call."""
    M = 3 * E + 5
    lset, rset = sets(3, 7, 2, 2)
    shape = (3, (M + 20) // 21, 7)
    M = shape[0] * shape[1] * shape[2]
    e = values(M, dt, 2)
    e[M // 2] = e[M // 2 + 100] = -1.0
    outs = []
    for op in (c_step, c_step, _hipops.minimize_step):
        ed = e.cuda()
        sd = [x.cuda() for x in state(dt, 5)]
        op(ed, *shape, lset.cuda(), rset.cuda(), *sd)
        outs.append([ed.cpu()] + [x.cpu() for x in sd])
    for other in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], other))
    assert outs[0][2].tolist() == expected_pos(M // 2, shape, lset, rset)


def ulp_probe(dt):
    g = torch.Generator().manual_seed(11)
    mag = 10 ** (torch.rand(1 << 20, generator=g, dtype=torch.float64) * 12 - 6)
    sign = torch.where(torch.rand(1 << 20, generator=g) < 0.5, -1.0, 1.0)
    return (mag * sign).to(dt)


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "fp64"])
def test_transformed_values_over_twelve_decades(dt):
    e = ulp_probe(dt)
    M = e.numel()
    lset, rset = sets(1, 1, 0, 0)
    for best in (None, -3.7):
        _, u = run(e, (1, M, 1), lset, rset, state(dt, 1, best=best))
        print("probe {} m0 = {}: largest deviation {} ulp (measured before: {})".format(dt, best or 0, u, ULP_MEASURED[dt]))


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "fp64"])
def test_refusals_leave_everything_untouched(dt):
    L = h.lib()
    code = h.dtype_code(dt)
    M = 105
    e = values(M, dt).cuda()
    keep = e.clone()
    lset, rset = (x.cuda() for x in sets(3, 7, 2, 2))
    best, pos, flags = (x.cuda() for x in state(dt, 5))
    need = L.ttr_minimize_workspace_bytes(code, M)
    ws = torch.empty(need, dtype=torch.uint8).cuda()
    ptr = lambda x: None if x is None else x.data_ptr()

    def call(dtype=code, e=e, Ra=3, I=5, Rb=7, ls=lset, ldl=3, nl=2, rs=rset, ldr=3, nr=2, best=best, pos=pos, flags=flags, wsp=ws, wsn=need):
        return L.ttr_minimize_step(dtype, ptr(e), Ra, I, Rb, ptr(ls), ldl, nl, ptr(rs), ldr, nr, ptr(best), ptr(pos), ptr(flags),
                                   ptr(wsp), wsn, None)

    assert L.ttr_minimize_workspace_bytes(7, M) == h.E_INVALID and L.ttr_minimize_workspace_bytes(code, 0) == h.E_INVALID
    assert call(dtype=7) == h.E_INVALID
    assert call(Ra=0) == h.E_INVALID and call(I=0) == h.E_INVALID and call(Rb=-1) == h.E_INVALID
    assert call(nl=-1) == h.E_INVALID and call(nr=-1) == h.E_INVALID and call(ldl=2) == h.E_INVALID and call(ldr=2) == h.E_INVALID
    for name in ("e", "ls", "rs", "best", "pos", "flags"):
        assert call(**{name: None}) == h.E_INVALID, name
    assert call(wsp=None) == h.E_WORKSPACE and call(wsn=need - 1) == h.E_WORKSPACE and call(wsn=0) == h.E_WORKSPACE
    assert call(I=1 << 55) == h.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(e, keep) and flags.tolist() == [0, 0] and pos.tolist() == [SENTINEL] * 5
    with pytest.raises(ValueError):
        h.minimize_step(e[::2], 1, 53, 1, lset[:1], rset[:1], best, pos, flags)
    with pytest.raises(ValueError):
        h.minimize_step(e, 3, 5, 7, lset, rset, best, pos[:4], flags)
    with pytest.raises(ValueError):
        h.minimize_step(e, 3, 5, 7, lset.int(), rset, best, pos, flags)
    assert call() == 0
    torch.cuda.synchronize()
    assert flags.tolist() == [1, 0] and float(best) == float(keep.min())


def test_workspace_and_symbols():
    wsb = h.minimize_workspace_bytes
    assert wsb(torch.float32, 1) == wsb(torch.float64, E) == 256          # one partial: 20 bytes, rounded up
    assert wsb(torch.float32, 100 * E + 1) == 101 * 20 + 256 - (101 * 20) % 256
    assert wsb(torch.float64, 1 << 40) == 2048 * 20                       # the grid is capped at 2048 workgroups
    for name in ("ttr_minimize_step", "ttr_minimize_workspace_bytes"):
        assert name in h.EXPORTED_SYMBOLS and hasattr(h.lib(), name)
    assert _hipops.MIN_BLOCK_ELEMS == E

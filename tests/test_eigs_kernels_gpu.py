"""``ttr_ritz_gram`` and ``ttr_ritz_update`` through the binding ``_hip``, on the device, in fp32 and fp64.

Bounds.  The Gram kernel adds exact (fp32 operands) or once-rounded (fp64) products in fp64, each sum one expression of at most
n + 1 additions, so an entry is within ``2 (n + 2) 2^-53 sum |a_i b_i|`` of the exact sum (Higham, section 3.1; the factor 2
covers the rounded products and the denominator).  The pencil's coefficients are held against the host mirror's within
``1e3 * 2^-53 / relgap`` (the sensitivity of an eigenvector is the perturbation over the gap; the pencils drawn here have a
relative Ritz gap of at least 0.1), and the updated vectors against the update evaluated in fp64 with the mirror's coefficients,
per element, within the rounding of the expression plus that coefficient term."""
import ctypes

import pytest
import torch

import eigs_cases as ec
from tntorch_amd import _hostops

pytestmark = pytest.mark.gpu

DTYPES = ec.DTYPES
U53 = 2.0 ** -53
INIT, STEP, SA, LA = _hostops.RITZ_INIT, _hostops.RITZ_STEP, _hostops.RITZ_SA, _hostops.RITZ_LA


def hip():
    from tntorch_amd import _hip

    return _hip


def sizes(dt):
    small, cap_n = ec.ritz_sizes(dt)
    return small + [cap_n, cap_n + 5]


def on_device(vs, offset=0):
    """Device copies of CPU vectors; ``offset`` elements in front of each, so that the views start off a 16-byte boundary."""
    out = []
    for v in vs:
        buf = torch.zeros(v.numel() + offset, dtype=v.dtype, device="cuda")
        buf[offset:] = v.cuda()
        out.append(buf[offset:])
    return out


def spread_vectors(n, dt, seed):
    """X, AX, W, AW, P, AP (CPU, dt) for A = diag(a), a rising from 0.5 to 2.5, with X heavy where a is small, W where it is
    large and P in the middle: the three Rayleigh quotients differ by O(1), so the pencil's gaps are not lost in the rounding of
    the sums however long the vectors are."""
    g = torch.Generator().manual_seed(7000 + 13 * seed + n % 1009)
    t = torch.linspace(0.0, 1.0, n, dtype=torch.float64) if n > 1 else torch.full((1,), 0.5, dtype=torch.float64)
    a = 0.5 + 2.0 * t
    draw = lambda: torch.randn(n, dtype=torch.float64, generator=g)  # noqa: E731
    X, W, P = draw() * (1.05 - t), draw() * (0.05 + t), draw() * (0.3 + t * (1 - t))
    return [v.to(dt) for v in (X, a * X, W, a * W, P, a * P)]


def norm64(v):
    """||v|| in fp64 from a pairwise sum of the squares: torch's CPU ``norm`` of 5e5 doubles is itself ~10 eps off (measured
    against ``math.fsum``), more than the bound it would be used to check."""
    v = v.double()
    return float(torch.sqrt((v * v).sum()))


def sym3(v):
    return _hostops._sym3(v)


def drawn_pencil(n, dt, which):
    """Vectors whose pencil has a relative Ritz gap >= 0.1 (fixed seeds, checked here on the CPU), the mirror's c, theta', kept
    and relgap for them from accurately summed Gram entries."""
    for seed in range(1, 30):
        vs = spread_vectors(n, dt, seed)
        val, _ = ec.gram64(*vs)
        c, theta, kept, relgap = _hostops.ritz_pencil(sym3(val[:6]), sym3(val[6:]), which, ec.eps(dt))
        if float(relgap) >= 0.1:
            return vs, c, float(theta), int(kept), float(relgap), val
    raise AssertionError("no pencil with a relative gap >= 0.1 among the seeds")


# ------------------------------------------------------------------ ritz_gram
@pytest.mark.parametrize("dt", DTYPES)
def test_parts_and_workspace(dt):
    h = hip()
    small, cap_n = ec.ritz_sizes(dt)
    V = 16 // (torch.finfo(dt).bits // 8)         # the elements of a 16-byte pack
    for n in small:
        assert h.ritz_parts(dt, n) == 1 + (-(-n // V) - 1) // 1024
    assert h.ritz_parts(dt, cap_n - 1) == 255 and h.ritz_parts(dt, cap_n) == 256 == h.RITZ_MAX_PARTS
    assert h.ritz_parts(dt, 100 * cap_n) == 256
    for n in (1, 4099, cap_n):
        assert h.ritz_workspace_bytes(dt, n) == 96 * h.ritz_parts(dt, n)


@pytest.mark.parametrize("dt", DTYPES)
def test_gram_against_fp64_sums(dt):
    h = hip()
    for n in sizes(dt):
        cpu = ec.ritz_vectors(n, dt, seed=3)
        dev, off = on_device(cpu), on_device(cpu, offset=1)
        assert all(v.data_ptr() % 16 == 0 for v in dev) and all(v.data_ptr() % 16 != 0 for v in off)
        for what, mode, args in (("init", INIT, (0, 1)), ("step without P", STEP, (0, 1, 2, 3)), ("step", STEP, (0, 1, 2, 3, 4, 5))):
            part = h.ritz_gram(mode, *[dev[i] for i in args])
            assert part.shape == (h.ritz_parts(dt, n), 12) and part.dtype == torch.float64
            val, mag = ec.gram64(*[cpu[i] for i in args])
            got = part.cpu().sum(0)
            bound = 2 * (n + 2) * U53 * mag
            worst = float(((got - val).abs() / bound.clamp_min(1e-300)).max())
            print("ritz_gram {} n = {} {}: largest error / bound = {:.4f}".format(what, n, dt, worst))
            assert bool(((got - val).abs() <= bound).all()), (what, n, worst)
            assert bool((got[mag == 0] == 0).all())                                  # the sums of a mode that does not read them
            again = h.ritz_gram(mode, *[dev[i] for i in args])
            assert torch.equal(part, again)                                          # the same call, the same bits
            shifted = h.ritz_gram(mode, *[off[i] for i in args])
            assert torch.equal(part, shifted)                                        # element loads, the same bits


# ------------------------------------------------------------------ ritz_update
def reference_update(cpu, c, theta, dt, has_p=True):
    """The step in fp64 with the given coefficients, and the magnitudes its bounds are made of."""
    X, AX, W, AW, P, AP = [v.double() for v in cpu]
    if not has_p:
        P, AP = torch.zeros_like(P), torch.zeros_like(AP)
    c0, c1, c2 = [float(v) for v in c]
    Pn, APn = c1 * W + c2 * P, c1 * AW + c2 * AP
    Xn, AXn = c0 * X + Pn, c0 * AX + APn
    Wn = AXn - theta * Xn
    mx = abs(c0) * X.abs() + abs(c1) * W.abs() + abs(c2) * P.abs()
    max_ = abs(c0) * AX.abs() + abs(c1) * AW.abs() + abs(c2) * AP.abs()
    sx, sax = X.abs() + W.abs() + P.abs(), AX.abs() + AW.abs() + AP.abs()
    return (Xn, AXn, Wn, Pn, APn), (mx, max_, sx, sax)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("which", [SA, LA])
def test_update_against_the_mirror(which, dt):
    h = hip()
    e = ec.eps(dt)
    for n in sizes(dt):       # (n = 1: X, W, P are parallel, one direction is kept and its relgap is 1)
        cpu, c, theta, kept, relgap, val = drawn_pencil(n, dt, which)
        for offset in (0, 1):
            dev = on_device(cpu, offset)
            state = torch.zeros(8, dtype=torch.float64, device="cuda")
            sweep = torch.zeros(4, dtype=torch.float64, device="cuda")
            part = h.ritz_gram(STEP, *dev)
            h.ritz_update(STEP, which, 1, 0.0, part, *dev, state, sweep)
            st = state.cpu()
            dc = 1e3 * U53 / relgap
            print("ritz_update n = {} {} which {} offset {}: relgap {:.3f}, c error {:.3e} (bound {:.3e}), kept {}".format(
                n, dt, which, offset, relgap, float((st[4:7] - c).abs().max()), dc, int(st[7])))
            assert float(st[2]) == 0 and float(st[3]) == 0 and int(st[7]) == kept == min(3, n)
            assert float((st[4:7] - c).abs().max()) <= dc and float(st[4]) >= 0
            (Xn, AXn, Wn, Pn, APn), (mx, max_, sx, sax) = reference_update(cpu, c, theta, dt)
            got = [v.double().cpu() for v in dev]
            dth = dc * abs(theta)      # for theta' alone: c^T T c with both c within dc, and the rounding of the sums
            assert abs(float(st[0]) - theta) <= dth + 8 * U53 * abs(theta)
            assert bool(((got[0] - Xn).abs() <= 4 * e * mx + dc * sx).all())
            assert bool(((got[1] - AXn).abs() <= 4 * e * max_ + dc * sax).all())
            assert bool(((got[4] - Pn).abs() <= 4 * e * mx + dc * sx).all())
            assert bool(((got[5] - APn).abs() <= 4 * e * max_ + dc * sax).all())
            assert bool(((got[2] - Wn).abs() <= 6 * e * (max_ + abs(theta) * mx) + dc * (sax + abs(theta) * sx)).all())
            assert torch.equal(got[3], cpu[3].double())                              # AW is read only
            assert abs(norm64(got[0]) - 1.0) <= 8 * e
            theta0 = float(val[6] / val[0])
            sign = 1.0 if which == SA else -1.0
            assert sign * (float(st[0]) - theta0) <= 8 * e * abs(theta0)
            res = float(torch.sqrt(val[3] / (val[3] + theta0 ** 2 * val[0])))
            assert abs(float(st[1]) - res) <= 1e-12 * res and float(sweep.cpu()[0]) == float(st[1]) and float(sweep.cpu()[2]) == float(st[0])


@pytest.mark.parametrize("dt", DTYPES)
def test_init_mode(dt):
    h = hip()
    e = ec.eps(dt)
    for n in (1, 257, 4099):
        for offset in (0, 1):
            cpu = ec.ritz_vectors(n, dt, seed=4)
            dev = on_device(cpu, offset)
            state = torch.zeros(8, dtype=torch.float64, device="cuda")
            sweep = torch.tensor([0.25, 0.0, 0.0, 0.0], dtype=torch.float64, device="cuda")
            h.ritz_update(INIT, SA, 0, 0.0, h.ritz_gram(INIT, dev[0], dev[1]), dev[0], dev[1], dev[2], None, dev[4], dev[5], state, sweep)
            X, AX = cpu[0].double(), cpu[1].double()
            nrm = norm64(X)
            theta = float(X @ AX) / nrm ** 2
            got = [v.double().cpu() for v in dev]
            st = state.cpu()
            assert abs(float(st[0]) - theta) <= 8 * U53 * (n + 2) * abs(theta) and float(st[3]) == 0 and float(st[7]) == 1
            assert bool(((got[0] - X / nrm).abs() <= 2 * e * (X / nrm).abs()).all())
            assert bool(((got[1] - AX / nrm).abs() <= 2 * e * (AX / nrm).abs()).all())
            assert bool(((got[2] - (got[1] - float(st[0]) * got[0])).abs() <= 2 * e * (got[1].abs() + abs(theta) * got[0].abs())).all())
            assert float(got[4].abs().max()) == 0 == float(got[5].abs().max()) and torch.equal(got[3], cpu[3].double())
            assert sweep.cpu().tolist() == [0.25, 0.0, float(st[0]), 0.0]


@pytest.mark.parametrize("dt", DTYPES)
def test_edge_pencils(dt):
    h = hip()
    n = 1023
    base = spread_vectors(n, dt, 1)

    def run(vs, rel=0.0, p=True, mode=STEP):
        dev = on_device(vs)
        state = torch.zeros(8, dtype=torch.float64, device="cuda")
        sweep = torch.zeros(4, dtype=torch.float64, device="cuda")
        if mode == INIT:
            part = h.ritz_gram(INIT, dev[0], dev[1])
        else:
            part = h.ritz_gram(STEP, dev[0], dev[1], dev[2], dev[3], dev[4] if p else None, dev[5] if p else None)
        h.ritz_update(mode, SA, 1, rel, part, dev[0], dev[1], dev[2], dev[3], dev[4] if p else None, dev[5] if p else None, state, sweep)
        return [v.cpu() for v in dev], state.cpu(), sweep.cpu()

    same = lambda got, vs: all(torch.equal(a, b) for a, b in zip(got, vs))  # noqa: E731
    finite = lambda got: all(bool(torch.isfinite(v).all()) for v in got)  # noqa: E731
    # frozen: rel above res; nothing is written, state[2] is set
    got, st, sw = run(base, rel=2.0)
    assert same(got, base) and float(st[2]) == 1 and 0 < float(st[1]) <= 1 and float(st[7]) == 0 and float(sw[0]) == float(st[1])
    # W = 0: frozen whatever rel is
    vs = [v.clone() for v in base]
    vs[2].zero_(), vs[3].zero_()
    got, st, _ = run(vs)
    assert same(got, vs) and float(st[2]) == 1 and float(st[1]) == 0 and float(st[7]) == 0 and finite(got)
    # P = None: two directions; P and AP are left alone
    got, st, _ = run(base, p=False)
    assert finite(got) and float(st[7]) == 2 and float(st[6]) == 0 and float(st[3]) == 0
    assert torch.equal(got[4], base[4]) and torch.equal(got[5], base[5])
    assert abs(norm64(got[0]) - 1.0) <= 8 * ec.eps(dt)
    # P = 2 W: one of the two is dropped
    vs = [v.clone() for v in base]
    vs[4], vs[5] = 2 * vs[2], 2 * vs[3]
    got, st, _ = run(vs)
    assert finite(got) and float(st[7]) == 2 and float(st[3]) == 0 and abs(norm64(got[0]) - 1.0) <= 8 * ec.eps(dt)
    # one element: the three directions are one
    one = [torch.tensor([v], dtype=dt) for v in (0.5, 0.75, -0.25, -0.375, 2.0, 3.0)]
    got, st, _ = run(one)
    assert finite(got) and float(st[7]) == 1 and abs(abs(float(got[0])) - 1.0) <= 8 * ec.eps(dt)
    # an inf in W: flag 1, nothing written
    vs = [v.clone() for v in base]
    vs[2][17] = float("inf")
    got, st, sw = run(vs)
    assert same(got, vs) and float(st[3]) == 1 and sw.tolist()[1:] == [1.0, 0.0, 1.0]
    # X = 0 in INIT: flag 2, nothing written
    vs = [v.clone() for v in base]
    vs[0].zero_(), vs[1].zero_()
    got, st, sw = run(vs, mode=INIT)
    assert same(got, vs) and float(st[3]) == 2 and sw.tolist()[1:] == [1.0, 0.0, 2.0] and float(st[7]) == 0


def test_sweep_accumulation():
    h = hip()
    dt = torch.float32
    base = spread_vectors(300, dt, 2)
    state = torch.zeros(8, dtype=torch.float64, device="cuda")
    sweep = torch.zeros(4, dtype=torch.float64, device="cuda")

    def step(vs, first):
        dev = on_device(vs)
        h.ritz_update(STEP, SA, first, 0.0, h.ritz_gram(STEP, *dev), *dev, state, sweep)
        return state.cpu().tolist(), sweep.cpu().tolist()

    st1, sw1 = step(base, 1)
    assert sw1 == [st1[1], 0.0, st1[0], 0.0] and st1[1] > 0
    small = [v.clone() for v in base]
    small[2] *= 0.5
    small[3] *= 0.5
    st2, sw2 = step(small, 1)                     # a smaller residual: the maximum stays
    assert 0 < st2[1] < st1[1] and sw2[0] == st1[1] and sw2[2] == st2[0]
    big = [v.clone() for v in base]
    big[2] *= 4.0
    big[3] *= 4.0
    st3, sw3 = step(big, 0)                       # first = 0: [0] is left alone
    assert st3[1] > st1[1] and sw3[0] == st1[1]
    st4, sw4 = step(big, 1)
    assert sw4[0] == st4[1] == st3[1]
    bad = [v.clone() for v in base]
    bad[1][3] = float("nan")
    for k in (1, 2):                              # [1] counts the flagged calls, [3] keeps their bits
        st, sw = step(bad, 1)
        assert st[3] == 1.0 and sw[1] == float(k) and sw[3] == 1.0 and sw[0] == st4[1]


def test_bad_arguments():
    """The header's error codes, before any launch."""
    h = hip()
    L = h.lib()
    x = torch.ones(64, dtype=torch.float32, device="cuda")
    part = torch.zeros(12, dtype=torch.float64, device="cuda")
    st = torch.zeros(8, dtype=torch.float64, device="cuda")
    p, q = x.data_ptr(), part.data_ptr()
    gram = lambda dtype=0, mode=1, n=64, X=p, AX=p, W=p, AW=p, P=None, AP=None, part_=q, wsb=96: L.ttr_ritz_gram(  # noqa: E731
        dtype, mode, n, X, AX, W, AW, P, AP, part_, wsb, None)
    upd = lambda dtype=0, mode=1, which=0, n=64, rel=0.0, part_=q, X=p, AW=p, P=None, AP=None, state=st.data_ptr(): L.ttr_ritz_update(  # noqa: E731
        dtype, mode, which, 1, n, rel, part_, X, p, p, AW, P, AP, state, st.data_ptr(), None)
    assert gram(dtype=7) == h.E_INVALID and gram(mode=2) == h.E_INVALID
    assert gram(n=0) == h.E_INVALID and b"n = 0 < 1" in L.ttr_last_error()
    assert gram(X=None) == h.E_INVALID and b"null pointer" in L.ttr_last_error()
    assert gram(W=None) == h.E_INVALID and gram(P=p) == h.E_INVALID and gram(part_=None) == h.E_INVALID
    assert gram(wsb=95) == h.E_WORKSPACE and b"96 needed" in L.ttr_last_error()
    assert gram(n=1 << 57, wsb=1 << 20) == h.E_UNSUPPORTED
    assert upd(dtype=7) == h.E_INVALID and upd(mode=2) == h.E_INVALID and upd(which=2) == h.E_INVALID
    assert upd(n=0) == h.E_INVALID and upd(n=-3) == h.E_INVALID and upd(rel=-1.0) == h.E_INVALID
    assert upd(X=None) == h.E_INVALID and upd(AW=None) == h.E_INVALID and upd(P=p) == h.E_INVALID
    assert upd(part_=None) == h.E_INVALID and upd(state=None) == h.E_INVALID
    assert L.ttr_ritz_parts(0, 0) == h.E_INVALID and L.ttr_ritz_workspace_bytes(7, 5) == h.E_INVALID
    torch.cuda.synchronize()
    assert float(part.abs().max()) == 0 and float(st.abs().max()) == 0 and bool((x == 1).all())     # nothing ran
    with pytest.raises(ValueError):
        h.ritz_gram(STEP, x[:0], x[:0], x[:0], x[:0])
    with pytest.raises(ValueError):
        h.ritz_gram(STEP, x, x.double(), x, x)

"""``ttr_sample_step`` through the binding on an MI355X, fp32 and fp64, against its definition in fp64 on the CPU: the tile, block
and rank edges, special thresholds, independence of the samples, layouts, flags and sentinels.

Bounds.  q is an inner product of r terms in the dtype, the running sum is fp64:
  X:    c_{x-1} - d <= u T < c_x + d  and  q_x > 0,  d = (r + 2) eps sum_i sum_a |L[p, a]| |fiber[a, i]| + I 2^-53 T
  Lnew: within (r + 2) eps sum_a |L[p, a]| |core[a, x, :]| / T of the fp64 value at the kernel's own x.
The bound on Lnew takes T as known to about an ulp of the dtype, which it is where q has no cancellation: L >= 0 and fiber >= 0
(``operands`` draws them so; the core is signed).  With signed L and fiber the computed T itself is only good to
(r + 2) eps sum_i S_i / T, S_i = sum_a |L[p, a]| |fiber[a, i]|, and the quotient inherits that: there (``signed=True``) the bound
on Lnew is (r + 2) eps (sum_a |L[p, a]| |core[a, x, :]| + |L[p, :] . core[:, x, :]| sum_i S_i / T) / T; the bound on X holds as it
stands, its d already carries S."""
import pytest
import torch

from tntorch_amd import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.float64]
SENT_X, SENT_L = -777, 12345.0


def tile(dtype):
    return _hip.sample_tile(dtype)   # (S, B)


def run(L, fiber, core, u, lnew=True):
    """One call on device copies of the operands, X and Lnew embedded in buffers with sentinels around them; returns
    (X, Lnew or None, flag word) on the CPU after checking the sentinels."""
    P, rn = L.shape[0], core.shape[2]
    Xb = torch.full((P + 2,), SENT_X, dtype=torch.int64, device=DEV)
    Lb = torch.full((P + 2, rn), SENT_L, dtype=core.dtype, device=DEV) if lnew else None
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    _hip.sample_step(L.to(DEV), fiber.to(DEV), core.to(DEV), u.to(DEV), Xb[1:P + 1], flag, Lb[1:P + 1] if lnew else None)
    Xb = Xb.cpu()
    assert Xb[0] == SENT_X and Xb[-1] == SENT_X
    if lnew:
        Lb = Lb.cpu()
        assert bool((Lb[0] == SENT_L).all()) and bool((Lb[-1] == SENT_L).all())
    return Xb[1:P + 1], (Lb[1:P + 1] if lnew else None), int(flag.item())


def row_sums(q):
    """sum_i q[:, i] with the rounding of every addition carried along (Neumaier): the truth's T is good to an ulp, so that
    the bound on Lnew measures the kernel and not this sum."""
    s, c = torch.zeros_like(q[:, 0]), torch.zeros_like(q[:, 0])
    for i in range(q.shape[1]):
        x = q[:, i]
        t = s + x
        c = c + torch.where(s >= x, (s - t) + x, (x - t) + s)
        s = t
    return s + c


def check(L, fiber, core, u, X, Lnew, tag, signed=False):
    """The bounds of the module docstring."""
    dtype = core.dtype
    eps = torch.finfo(dtype).eps
    r, I, rn = core.shape
    Ld, fd, cd = L.double(), fiber.double(), core.double()
    q = (Ld @ fd).abs()
    S = Ld.abs() @ fd.abs()
    c = torch.cumsum(q, dim=1)
    T = row_sums(q)
    d = (r + 2) * eps * S.sum(dim=1) + I * 2.0 ** -53 * T
    assert bool(((X >= 0) & (X < I)).all()), tag
    cx = c.gather(1, X[:, None])[:, 0]
    qx = q.gather(1, X[:, None])[:, 0]
    cprev = cx - qx if I == 1 else torch.where(X > 0, c.gather(1, (X - 1).clamp_min(0)[:, None])[:, 0], torch.zeros_like(cx))
    uT = u * T
    assert bool((qx > 0).all()), tag
    assert bool((cprev - d <= uT).all()) and bool((uT < cx + d).all()), tag
    if Lnew is not None:
        G = cd[:, X, :]                                                # [r, P, rn]
        want = torch.einsum("pa,apb->pb", Ld, G) / T[:, None]
        bound = (r + 2) * eps * torch.einsum("pa,apb->pb", Ld.abs(), G.abs()) / T[:, None]
        if signed:
            bound = bound + (r + 2) * eps * want.abs() * (S.sum(dim=1) / T)[:, None]
        else:
            assert bool((Ld >= 0).all()) and bool((fd >= 0).all())
        err = (Lnew.double() - want).abs()
        assert bool((err <= bound).all()), "{}: Lnew off by {:.3e} of its bound".format(tag, float((err / bound).max()))


def operands(P, r, I, rn, dtype, seed, signed=False):
    """L and fiber uniform in [0, 1) (normal when ``signed``), a normal core: the entry takes fiber as an input of its own."""
    g = torch.Generator().manual_seed(seed)
    draw = torch.randn if signed else torch.rand
    L = draw((P, r), generator=g, dtype=torch.float64).to(dtype)
    core = torch.randn((r, I, rn), generator=g, dtype=torch.float64).to(dtype)
    fiber = draw((r, I), generator=g, dtype=torch.float64).to(dtype)
    u = torch.rand((P,), generator=g, dtype=torch.float64)
    return L, fiber, core, u


RANKS = [1, 3, 17, 33, None]   # None: ttr_sample_max_rank()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rn", RANKS)
@pytest.mark.parametrize("r", RANKS)
def test_shapes(r, rn, dtype):
    S, B = tile(dtype)
    r, rn = r or _hip.sample_max_rank(), rn or _hip.sample_max_rank()
    Is = [1, B - 1, B, B + 1, 2 * B + 1] + ([4096] if r == 3 and rn == 3 else [])
    for I in Is:
        for P in (1, S - 1, S, S + 1, 2 * S + 3):
            L, fiber, core, u = operands(P, r, I, rn, dtype, 1000 * r + 10 * rn + I % 7)
            tag = "P={} r={} I={} rn={} {}".format(P, r, I, rn, dtype)
            X, Lnew, word = run(L, fiber, core, u)
            assert word == 0, tag
            check(L, fiber, core, u, X, Lnew, tag)
            if P == S + 1:   # signed L and fiber: |q| of sums that cancel
                L, fiber, core, u = operands(P, r, I, rn, dtype, 1000 * r + 10 * rn + I % 7, signed=True)
                X, Lnew, word = run(L, fiber, core, u)
                assert word == 0, tag
                check(L, fiber, core, u, X, Lnew, tag + " signed", signed=True)
            if rn == 1:   # the last mode: no Lnew, the same X
                X2, none, word = run(L, fiber, core, u, lnew=False)
                assert none is None and word == 0 and torch.equal(X, X2), tag


@pytest.mark.parametrize("dtype", DTYPES)
def test_extreme_thresholds(dtype):
    S, B = tile(dtype)
    P, r, I, rn = S + 1, 3, 2 * B + 1, 3
    L, fiber, core, _ = operands(P, r, I, rn, dtype, 5)
    L, fiber = L + 0.5, fiber + 0.5
    q = (L.double() @ fiber.double()).abs()
    assert bool((q > 0).all())
    for u, want in ((0.0, 0), (1 - 2.0 ** -53, I - 1)):
        uu = torch.full((P,), u, dtype=torch.float64)
        X, Lnew, word = run(L, fiber, core, uu)
        assert word == 0 and bool((X == want).all())
        check(L, fiber, core, uu, X, Lnew, "u = {}".format(u))


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_mass_at_the_ends_is_never_chosen(dtype):
    """Integer-valued q (exact in either dtype) with exactly zero leading and trailing columns, across a block edge at the end."""
    S, B = tile(dtype)
    P, r, I, rn = S + 1, 3, 2 * B + 1, 2
    g = torch.Generator().manual_seed(9)
    L = torch.randint(1, 4, (P, r), generator=g).to(dtype)
    fiber = torch.randint(1, 4, (r, I), generator=g).to(dtype)
    fiber[:, :3] = 0
    fiber[:, B - 2:] = 0   # the whole second and third block, and the end of the first
    core = torch.randn((r, I, rn), generator=g, dtype=torch.float64).to(dtype)
    for u, want in ((0.0, 3), (1 - 2.0 ** -53, B - 3)):
        X, _, word = run(L, fiber, core, torch.full((P,), u, dtype=torch.float64))
        assert word == 0 and bool((X == want).all()), (u, X)
    u = torch.rand((P,), generator=g, dtype=torch.float64)
    X, Lnew, word = run(L, fiber, core, u)
    assert word == 0 and bool(((X >= 3) & (X <= B - 3)).all())
    check(L, fiber, core, u, X, Lnew, "zero ends")


@pytest.mark.parametrize("dtype", DTYPES)
def test_threshold_on_a_boundary(dtype):
    """q = 3 in every column, I a power of two: c_i = 3 (i + 1), T = 3 I and u = k / I are exact, u T = c_{k-1}.  The strict
    inequality takes x = k, the next smaller threshold x = k - 1: at every column, so at every segment and block boundary."""
    S, B = tile(dtype)
    I = 4 * B
    L = torch.ones((I, 3), dtype=dtype)
    fiber = torch.ones((3, I), dtype=dtype)
    core = torch.ones((3, I, 2), dtype=dtype)
    u = torch.arange(I, dtype=torch.float64) / I
    X, Lnew, word = run(L, fiber, core, u)
    assert word == 0 and torch.equal(X, torch.arange(I))
    assert torch.equal(Lnew, torch.full((I, 2), 3.0 / (3 * I), dtype=dtype))
    below = torch.nextafter(u[1:], torch.zeros(I - 1, dtype=torch.float64))
    X, _, word = run(L[1:], fiber, core, below)
    assert word == 0 and torch.equal(X, torch.arange(I - 1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_samples_are_independent_and_calls_repeat(dtype):
    S, B = tile(dtype)
    P, r, I, rn = 2 * S + 3, 17, 2 * B + 1, 5
    L, fiber, core, u = operands(P, r, I, rn, dtype, 21)
    X, Lnew, word = run(L, fiber, core, u)
    X2, Lnew2, _ = run(L, fiber, core, u)
    assert word == 0 and torch.equal(X, X2) and torch.equal(Lnew.view(torch.uint8), Lnew2.view(torch.uint8))
    for k in (1, S, S + 1):
        Xk, Lk, _ = run(L[:k], fiber, core, u[:k])
        assert torch.equal(Xk, X[:k]) and torch.equal(Lk.contiguous().view(torch.uint8), Lnew[:k].contiguous().view(torch.uint8)), k
    # a sample's result does not depend on its place in a tile: the samples in reverse order
    Xr, Lr, _ = run(L.flip(0), fiber, core, u.flip(0))
    assert torch.equal(Xr.flip(0), X) and torch.equal(Lr.flip(0), Lnew)


@pytest.mark.parametrize("dtype", DTYPES)
def test_layouts(dtype):
    S, B = tile(dtype)
    P, r, I, rn, N = S + 1, 3, B + 1, 5, 3
    L, fiber, core, u = operands(P, r, I, rn, dtype, 33)
    X0, L0, word = run(L, fiber, core, u)
    assert word == 0
    Lw = torch.full((P, r + 3), 7.0, dtype=dtype, device=DEV)
    Lw[:, :r] = L.to(DEV)
    Un = torch.full((P, N), 0.5, dtype=torch.float64, device=DEV)
    Un[:, 1] = u.to(DEV)
    Xs = torch.full((P, N), SENT_X, dtype=torch.int64, device=DEV)
    Ln = torch.full((P, rn + 2), SENT_L, dtype=dtype, device=DEV)
    wide = torch.full((r, 2 * I, rn + 1), 9.0, dtype=dtype, device=DEV)
    wide[:, ::2, :rn] = core.to(DEV)
    cview = wide[:, ::2, :rn]
    assert not cview.is_contiguous() and cview.stride(2) == 1
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    _hip.sample_step(Lw[:, :r], fiber.to(DEV), cview, Un[:, 1], Xs[:, 1], flag, Ln[:, :rn])
    assert int(flag.item()) == 0
    Xs, Ln = Xs.cpu(), Ln.cpu()
    assert torch.equal(Xs[:, 1], X0) and bool((Xs[:, 0] == SENT_X).all()) and bool((Xs[:, 2] == SENT_X).all())
    assert torch.equal(Ln[:, :rn], L0) and bool((Ln[:, rn:] == SENT_L).all())
    x = torch.full((P,), SENT_X, dtype=torch.int64, device=DEV)
    with pytest.raises(NotImplementedError):   # a core whose last stride is not 1
        _hip.sample_step(L.to(DEV), fiber.to(DEV), core.permute(2, 1, 0).contiguous().permute(2, 1, 0).to(DEV), u.to(DEV), x, flag, None)
    assert bool((x == SENT_X).all())
    with pytest.raises(ValueError):            # a rank above the limit
        big = _hip.sample_max_rank() + 1
        _hip.sample_step(torch.ones((P, big), dtype=dtype, device=DEV), torch.ones((big, I), dtype=dtype, device=DEV),
                         torch.ones((big, I, rn), dtype=dtype, device=DEV), u.to(DEV), x, flag, None)
    assert bool((x == SENT_X).all()) and int(flag.item()) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_flags(dtype):
    S, B = tile(dtype)
    P, r, I, rn = S + 5, 3, B + 1, 4
    L, fiber, core, u = operands(P, r, I, rn, dtype, 44)
    X0, L0, word = run(L, fiber, core, u)
    assert word == 0
    defects = {2: ("zero", _hip.SAMPLE_ZERO_TOTAL), 5: ("inf", _hip.SAMPLE_NONFINITE), S: ("one", _hip.SAMPLE_BAD_THRESHOLD),
               S + 3: ("nan", _hip.SAMPLE_BAD_THRESHOLD)}

    def spoil(rows):
        Lb, ub = L.clone(), u.clone()
        for p in rows:
            kind = defects[p][0]
            if kind == "zero":
                Lb[p] = 0
            elif kind == "inf":
                Lb[p, 1] = float("inf")
            elif kind == "one":
                ub[p] = 1.0
            else:
                ub[p] = float("nan")
        return Lb, ub

    for rows in [[p] for p in defects] + [list(defects)]:
        Lb, ub = spoil(rows)
        X, Ln, word = run(Lb, fiber, core, ub)
        want = 0
        for p in rows:
            want |= defects[p][1]
        assert word == want, (rows, word)
        keep = torch.ones(P, dtype=torch.bool)
        keep[rows] = False
        assert bool((X[~keep] == -1).all()) and bool((Ln[~keep] == 0).all())
        assert torch.equal(X[keep], X0[keep]) and torch.equal(Ln[keep], L0[keep])

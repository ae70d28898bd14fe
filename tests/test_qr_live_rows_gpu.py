"""The 8-wave pair kernel of qr_factor runs its panel chain over a block's LIVE rows only (blocks of 257 .. 384 rows; level 1 of
packed items in launches of >= 256 items): rows that are exactly zero are neither multiplied nor summed.  Every dropped term is an exact 0 * x or x + 0 and the sums keep their order over the
remaining terms, so the results must be EQUAL (torch.equal: -0 == +0), not close, to those of the code path that carries the
zeros along -- the zero-padded twin of a short block, or the same launch with bit 1 of TTR_KNOB_QR_PACK_PRE set.

Which cases run live-row code: m > 256 under "pair-steps" (m <= 384: the 6-group instance), test_short_block_on_the_pair_kernel
(4-group instance), the 350-row and 320-row blocks of the LAPACK / five-leaves cases under "pair-steps", and the B = 256 packed
level 1.  The 4-wave kernel (m <= 256), every "single-steps" case, the B = 3 packed case and the 130-train round_tt compare a
code path that has no live-row variant with itself: they pin down that the switch and the short path stay without effect there."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DT = [torch.float32, torch.float64]


def tol(dt, f32, f64):
    return f32 if dt == torch.float32 else f64


def _hip():
    from tntorch_amd import _hip

    _hip.lib()
    return _hip


@pytest.fixture(params=[1, 0], ids=["pair-steps", "single-steps"])
def qr_variant(request):
    h = _hip()
    h.set_knob(h.KNOB_QR_PANEL, request.param)
    yield request.param
    h.set_knob(h.KNOB_QR_PANEL, 1)


def _short_against_padded(h, A, mp):
    """A [B, m, n] takes the short path of its block, [A; 0] (mp rows: a whole block) the full one."""
    B, m, n = A.shape
    Ap = torch.cat([A, torch.zeros(B, mp - m, n, dtype=A.dtype)], dim=1)
    f, fp = h.qr_factor(A.cuda()), h.qr_factor(Ap.cuda())
    assert torch.equal(f.R, fp.R)
    Q, Qp = h.qr_apply(f), h.qr_apply(fp)
    assert torch.equal(Q, Qp[:, :m])
    assert torch.equal(Qp[:, m:], torch.zeros_like(Qp[:, m:]))
    return f, Q


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", [64, 33, 16])
@pytest.mark.parametrize("m", [64, 65, 128, 129, 192, 193, 255, 257, 320, 384, 385, 448, 511])
def test_short_block_equals_its_zero_padded_twin(dt, m, n, qr_variant):
    """One block of m rows (4 waves up to 256 rows, 8 above) against the same matrix padded with zero rows to the whole block, both
    sides of every 64-row boundary.  Only the 8-wave pair kernel has live-row instances (m = 257 .. 384: six of eight groups)."""
    h = _hip()
    g = torch.Generator().manual_seed(m * 31 + n)
    A = torch.randn(2, m, n, generator=g, dtype=torch.float64).to(dt)
    f, Q = _short_against_padded(h, A, 256 if m <= 256 else 512)
    # (and it is a QR factorisation: the bounds of test_qr)
    Q, R = Q.cpu().double(), f.R.cpu().double()
    assert (Q.transpose(1, 2) @ Q - torch.eye(n, dtype=torch.float64)).abs().max() < tol(dt, 2e-5, 5e-13)
    assert (Q @ R - A.double()).abs().max() / A.abs().max() < tol(dt, 1e-5, 1e-13)


@pytest.mark.parametrize("m", [64, 65, 129, 193])
def test_short_block_on_the_pair_kernel(m):
    """fp32 matrices of <= 256 rows on the 8-wave pair kernel (bit 2 of TTR_KNOB_QR_F64_NW4): the instance for two live row pairs of
    four (the smallest there is); the twin is padded to the kernel's 512 rows."""
    h = _hip()
    g = torch.Generator().manual_seed(m)
    A = torch.randn(2, m, 64, generator=g, dtype=torch.float32)
    h.set_knob(h.KNOB_QR_F64_NW4, 4)
    try:
        _short_against_padded(h, A, 512)
    finally:
        h.set_knob(h.KNOB_QR_F64_NW4, 0)


@pytest.mark.parametrize("dt", DT)
def test_first_core_of_a_sum(dt, qr_variant):
    """[G, G], 64 x 64 of rank 32: the first core of g + g -- a 64-row block whose trailing panels are rounding noise."""
    h = _hip()
    g = torch.Generator().manual_seed(11)
    G = torch.randn(2, 64, 32, generator=g, dtype=torch.float64)
    A = torch.cat([G, G], dim=2).to(dt)
    f, Q = _short_against_padded(h, A, 256)
    assert (Q.cpu().double() @ f.R.cpu().double() - A.double()).abs().max() / A.abs().max() < tol(dt, 1e-5, 1e-13)


@pytest.mark.parametrize("dt", DT)
def test_two_short_blocks_against_lapack(dt, qr_variant):
    """m = 700: two blocks of 350 rows (three live quarters of the 512-row block) and a 128-row top level; the bounds of test_qr."""
    h = _hip()
    m, n = 700, 64
    g = torch.Generator().manual_seed(m * 31 + n)
    A = torch.randn(2, m, n, generator=g, dtype=torch.float64).to(dt)
    Q, R = h.qr(A.cuda())
    Q, R = Q.cpu().double(), R.cpu().double()
    assert (Q.transpose(1, 2) @ Q - torch.eye(n, dtype=torch.float64)).abs().max() < tol(dt, 2e-5, 5e-13)
    assert (Q @ R - A.double()).abs().max() / A.abs().max() < tol(dt, 1e-5, 1e-13)
    assert R.tril(-1).abs().max() == 0
    Rref = torch.linalg.qr(A.double())[1]
    assert (R.abs() - Rref.abs()).abs().max() / Rref.abs().max() < tol(dt, 2e-4, 1e-11)


def _packed_inputs(B, dt, device, full_rank_item):
    """As test_qr_pushed_rank_deficient_R_packs_rows (k = Rin = n = 64, I = 64): R factors of numerical rank 32 and a core with the
    block structure of g + g; item `full_rank_item` has a full-rank R (it does not pack)."""
    g = torch.Generator(device=device).manual_seed(B)
    I = 64
    rnd = lambda *s: torch.randn(*s, generator=g, device=device, dtype=torch.float64)
    low = 1e-9 if dt == torch.float32 else 1e-18   # rows 32 .. 63 below 8 eps of the block in the format under test: the item packs
    Rm = torch.cat([torch.triu(rnd(B, 32, 64)), low * torch.triu(rnd(B, 32, 64), diagonal=32)], dim=1)
    Rm[full_rank_item] = torch.triu(rnd(64, 64))
    gcore = rnd(B, 32, I, 32).to(dt)
    z = torch.zeros_like(gcore)
    core = torch.cat([torch.cat([gcore, z], dim=-1), torch.cat([z, gcore], dim=-1)], dim=1)
    return Rm.to(dt), core


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("B", [3, 256])   # 256: the smallest batch that takes the packing flags ahead of the launch
def test_level1_of_packed_items_switch_on_equals_switch_off(dt, B):
    """Level 1 above a packed level 0: rows 256 .. 511 of a packed item's stacked R are the absorbed leaves' zero blocks.  The
    launch decides per item (one item of the batch has full rank and keeps all its rows); with bit 1 of TTR_KNOB_QR_PACK_PRE the
    zero rows are treated as ordinary rows by factor and apply alike."""
    h = _hip()
    Rm, core = _packed_inputs(B, dt, "cuda", 1)
    eye = torch.eye(64, dtype=dt, device="cuda")[None].repeat(B, 1, 1)
    res = {}
    for knob in (1, 3):
        h.set_knob(h.KNOB_QR_PACK_PRE, knob)
        f = h.qr_factor_pushed(Rm, core)
        res[knob] = (f.R.clone(), f.rows32.clone(), h.qr_apply(f, eye[:, :, :32].contiguous()), h.qr_apply(f, eye[:, :, 32:].contiguous()))
    h.set_knob(h.KNOB_QR_PACK_PRE, 1)
    flags = res[1][1].cpu()
    assert int(flags[1]) == 0 and bool((flags[torch.arange(B) != 1] == 3).all())   # (the case is what it claims to be)
    for a, b in zip(res[1], res[3]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dt", DT)
def test_level1_with_five_leaves(dt, qr_variant):
    """I = 40: five leaves, never packed, a 320-row level-1 block (three live quarters); the bounds of test_qr_pushed."""
    h = _hip()
    k, Rin, I, n, B = 64, 64, 40, 64, 2
    g = torch.Generator().manual_seed(k * 1000 + Rin * 100 + I * 10 + n)
    Rm = torch.randn(B, k, Rin, generator=g, dtype=torch.float64).to(dt)
    core = torch.randn(B, Rin, I, n, generator=g, dtype=torch.float64).to(dt)
    P = (Rm.double() @ core.double().reshape(B, Rin, I * n)).reshape(B, k * I, n)
    f = h.qr_factor_pushed(Rm.cuda(), core.cuda())
    Q = h.qr_apply(f).cpu().double()
    R = f.R.cpu().double()
    assert (Q.transpose(1, 2) @ Q - torch.eye(n, dtype=torch.float64)).abs().max() < tol(dt, 3e-5, 1e-12)
    assert (Q @ R - P).abs().max() / P.abs().max() < tol(dt, 2e-5, 1e-12)
    Rref = torch.linalg.qr(P)[1]
    assert (R.abs() - Rref.abs()).abs().max() / Rref.abs().max() < tol(dt, 3e-4, 1e-10)


def test_round_tt_equal_cores_under_both_switch_values():
    """round_tt(rmax=32) of 130 trains shaped like the headline's (64^8, t = g + g, g of rank 32): equal cores."""
    import tntorch_amd as tn

    h = _hip()
    B, N, mode, r = 130, 8, 64, 32
    gen = torch.Generator(device="cuda").manual_seed(5)
    ranks = [1] + [r] * (N - 1) + [1]
    inp = []
    for k in range(N):
        gk = torch.randn((B, ranks[k], mode, ranks[k + 1]), generator=gen, device="cuda", dtype=torch.float32)
        if k == 0:
            c = torch.cat([gk, gk], dim=-1)
        elif k == N - 1:
            c = torch.cat([gk, gk], dim=-3)
        else:
            z = torch.zeros_like(gk)
            c = torch.cat([torch.cat([gk, z], dim=-1), torch.cat([z, gk], dim=-1)], dim=-3)
        inp.append(c.contiguous())
    out = {}
    for knob in (1, 3):
        h.set_knob(h.KNOB_QR_PACK_PRE, knob)
        t = tn.Tensor([c.clone() for c in inp], batch=True)
        t.round_tt(rmax=r)
        torch.cuda.synchronize()
        out[knob] = [c.clone() for c in t.cores]
    h.set_knob(h.KNOB_QR_PACK_PRE, 1)
    assert tuple(out[1][1].shape) == (B, r, mode, r)
    for a, b in zip(out[1], out[3]):
        assert torch.equal(a, b)

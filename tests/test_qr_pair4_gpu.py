"""The FOUR-wave instance of qr_factor's pair kernel (TTR_KNOB_QR_PAIR4): a 256-row block of four waves, each owning two column
pairs of the panel, in place of the 8-wave instance for four live row groups -- level 1 of the packed items of a launch of >= 256
items by default, plain fp32 matrices of <= 256 rows and more than 32 columns with bit 1 of the knob.  It performs the same
arithmetic in the same order, so every comparison against the 8-wave instance is torch.equal, not a tolerance:

  * the level-1 switch: knob 1 against knob 0 on packed pushed factorisations (R, the rows32 flags, qr_apply of both halves of I);
  * plain matrices under bit 1 against the 8-wave instance (bit 2 of TTR_KNOB_QR_F64_NW4): every 64-row boundary, a last pair of one
    column (odd n), ragged column tiles (n = 33); Q is formed by the 4-wave apply kernel from the 256-row reflector layout;
  * rank edges on either side of a panel boundary, the larfg floor, the range guard;
  * round_tt end to end (the top level's exponent bookkeeping, the apply side on the 512-row layout)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _hip():
    from tntorch_amd import _hip

    _hip.lib()
    return _hip


def _factor_plain(h, A, four_wave):
    """R and Q of A [B, m, n] (fp32, m <= 256): on the four-wave pair instance, or on its 8-wave twin."""
    h.set_knob(h.KNOB_QR_PAIR4, 3 if four_wave else 1)
    h.set_knob(h.KNOB_QR_F64_NW4, 0 if four_wave else 4)
    try:
        f = h.qr_factor(A)
        Q = h.qr_apply(f)
        torch.cuda.synchronize()
        return f.R.clone(), Q.clone()
    finally:
        h.set_knob(h.KNOB_QR_PAIR4, 1)
        h.set_knob(h.KNOB_QR_F64_NW4, 0)


def _packed_inputs(B, full_rank_item):
    """k = Rin = n = I = 64 in fp32: R factors of numerical rank 32 (rows 32 .. 63 below 8 eps of the block: the item packs) and a
    core with the block structure of g + g; item `full_rank_item` has a full-rank R and keeps all its rows."""
    g = torch.Generator(device="cuda").manual_seed(B)
    I = 64
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda", dtype=torch.float64)
    Rm = torch.cat([torch.triu(rnd(B, 32, 64)), 1e-9 * torch.triu(rnd(B, 32, 64), diagonal=32)], dim=1)
    Rm[full_rank_item] = torch.triu(rnd(64, 64))
    gcore = rnd(B, 32, I, 32).float()
    z = torch.zeros_like(gcore)
    core = torch.cat([torch.cat([gcore, z], dim=-1), torch.cat([z, gcore], dim=-1)], dim=1)
    return Rm.float(), core


@pytest.mark.parametrize("B", [256, 257])
def test_level1_switch_on_equals_switch_off(B):
    """Level 1 above a packed level 0, in launches that decide per item (>= 256 items; one item has full rank and stays on the full
    8-wave instance): the packed items on the four-wave instance (knob 1) against the 8-wave instance for four live groups (knob 0)."""
    h = _hip()
    Rm, core = _packed_inputs(B, 1)
    eye = torch.eye(64, dtype=torch.float32, device="cuda")[None].repeat(B, 1, 1)
    res = {}
    try:
        for knob in (1, 0):
            h.set_knob(h.KNOB_QR_PAIR4, knob)
            f = h.qr_factor_pushed(Rm, core)
            res[knob] = (f.R.clone(), f.rows32.clone(), h.qr_apply(f, eye[:, :, :32].contiguous()), h.qr_apply(f, eye[:, :, 32:].contiguous()))
    finally:
        h.set_knob(h.KNOB_QR_PAIR4, 1)
    flags = res[1][1].cpu()
    assert int(flags[1]) == 0 and bool((flags[torch.arange(B) != 1] == 3).all())   # (the case is what it claims to be)
    for a, b in zip(res[1], res[0]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("n", [64, 63, 48, 33])
@pytest.mark.parametrize("m", [64, 65, 129, 193, 255, 256])
def test_plain_matrix_equals_the_eight_wave_instance(m, n):
    h = _hip()
    g = torch.Generator().manual_seed(m * 31 + n)
    A = torch.randn(2, m, n, generator=g, dtype=torch.float64).float()
    R4, Q4 = _factor_plain(h, A.cuda(), True)
    R8, _ = _factor_plain(h, A.cuda(), False)
    assert torch.equal(R4, R8)
    # (and it is a QR factorisation: the bounds of test_short_block_equals_its_zero_padded_twin)
    Q, R = Q4.cpu().double(), R4.cpu().double()
    assert (Q.transpose(1, 2) @ Q - torch.eye(n, dtype=torch.float64)).abs().max() < 2e-5
    assert (Q @ R - A.double()).abs().max() / A.abs().max() < 1e-5


def _rank_edge_cases():
    g = torch.Generator().manual_seed(7)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    G = rnd(2, 64, 32)
    cases = {"first-core": torch.cat([G, G], dim=2)}   # [G, G], 64 x 64 of rank 32: the first core of g + g
    for r in (15, 16, 17, 31, 33):                     # the skip decision on either side of a panel boundary
        cases[f"rank{r}"] = rnd(2, 200, r) @ rnd(2, r, 64)
    cases["zero"] = torch.zeros(2, 130, 64, dtype=torch.float64)        # larfg floor
    cases["up40"] = rnd(2, 200, 64) * 2.0 ** 40                         # range guard and exponent
    cases["down40"] = rnd(2, 200, 64) * 2.0 ** -40
    return cases


_CASES = _rank_edge_cases()


@pytest.mark.parametrize("name", list(_CASES))
def test_rank_edges_equal_the_eight_wave_instance(name):
    h = _hip()
    A = _CASES[name].float().cuda()
    R4, _ = _factor_plain(h, A, True)
    R8, _ = _factor_plain(h, A, False)
    assert torch.isfinite(R4).all()
    assert torch.equal(R4, R8)


def test_round_tt_equal_cores_under_both_switch_values():
    """round_tt(rmax=32) of 256 trains g + g with four 64-mode cores (g of rank 32): every output core equal."""
    import tntorch_amd as tn

    h = _hip()
    B, N, mode, r = 256, 4, 64, 32
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
    try:
        for knob in (1, 0):
            h.set_knob(h.KNOB_QR_PAIR4, knob)
            t = tn.Tensor([c.clone() for c in inp], batch=True)
            t.round_tt(rmax=r)
            torch.cuda.synchronize()
            out[knob] = [c.clone() for c in t.cores]
    finally:
        h.set_knob(h.KNOB_QR_PAIR4, 1)
    assert tuple(out[1][1].shape) == (B, r, mode, r)
    for a, b in zip(out[1], out[0]):
        assert torch.equal(a, b)

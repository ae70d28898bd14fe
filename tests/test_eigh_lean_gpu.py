"""The large-launch builds of the 32-row top-r eigensolver (TTR_KNOB_EIGH_SMALL = 2 / 3: launches of >= 1024 fp32 matrices; 3 is
the lean 128-register instance with the pivots of the twisted factorisation in LDS) against the spill-free build that serves every
size (1): same bits, on both sides of the dispatch threshold, for every kind of item in one batch."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

BMAX, N, K = 1031, 64, 96
PAIR, ZERO = 3, 9      # items with close eigenvalue pairs / all zeros (neither graded nor full-size below)


def _hip():
    from tntorch_amd import _hip

    _hip.lib()
    return _hip


@functools.lru_cache(maxsize=None)
def _partials():
    """[BMAX, 4, 64, 64] fp32 on the device: four split-K partials of the Gram matrices of one batch of rows (float64 on the host)."""
    g = torch.Generator().manual_seed(77)
    rows = torch.zeros(BMAX, N, K, dtype=torch.float64)
    rows[:, :32] = torch.randn(BMAX, 32, K, generator=g, dtype=torch.float64)                       # flat, zero tail
    rows[::7, :32] *= (2.0 ** (-torch.arange(32, dtype=torch.float64)))[None, :, None]               # graded: declined, QL in the same launch
    rows[5::11, 40] = 0.5 * torch.randn(len(range(5, BMAX, 11)), K, generator=g, dtype=torch.float64)  # no zero tail: the 64-row launch
    # eigenvalue pairs 100 eps lambda_1 apart (closer than the admitted 512 eps lambda_1)
    e = torch.finfo(torch.float32).eps
    Q = torch.linalg.qr(torch.randn(32, 32, generator=g, dtype=torch.float64))[0]
    sig = torch.tensor([(1.0 - 0.02 * (i // 2)) * (1.0 + 50 * e * (i % 2)) for i in range(32)], dtype=torch.float64)
    rows[PAIR] = 0
    rows[PAIR, :32, :32] = Q * sig
    rows[ZERO] = 0
    parts = torch.stack([rows[:, :, 24 * p:24 * (p + 1)] @ rows[:, :, 24 * p:24 * (p + 1)].transpose(1, 2) for p in range(4)], dim=1)
    return parts.to(torch.float32).cuda()


@pytest.mark.parametrize("parts", [1, 4])
@pytest.mark.parametrize("r", [8, 32])
@pytest.mark.parametrize("B", [1023, 1024, 1031])
def test_large_launch_builds_of_the_32_row_top_r_kernel_give_the_bits_of_the_spill_free_build(B, r, parts):
    h = _hip()
    P = _partials()[:B]
    G = P.contiguous() if parts == 4 else P.sum(dim=1)
    out = {}
    try:
        for v in (1, 2, 3):
            h.set_knob(h.KNOB_EIGH_SMALL, v)
            out[v] = [x.clone() for x in h.eigh_top(G, r, 0.125)]
    finally:
        h.set_knob(h.KNOB_EIGH_SMALL, 2)
    V, sigma, info, flat = out[1]
    # every kind of item is there: taken by the top-r path, declined (graded, close pairs), full-size, zero
    graded = torch.zeros(B, dtype=torch.bool)
    graded[::7] = True
    full = torch.zeros(B, dtype=torch.bool)
    full[5::11] = True
    fl = flat.cpu()
    plain = ~graded & ~full
    plain[[PAIR, ZERO]] = False
    assert bool((fl[plain] == 1).all()) and int(plain.sum()) > B // 2
    assert bool((fl[graded & ~full] != 1).all()) and int(fl[PAIR]) != 1
    assert bool((sigma[plain.cuda()][:, r:] == 0).all()) and not bool(sigma[ZERO].any())
    for v in (2, 3):
        for name, a, b in zip(("V", "sigma", "info", "flat"), out[1], out[v]):
            assert torch.equal(a, b), (v, name)

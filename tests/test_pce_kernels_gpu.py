"""ttr_pce_design and ttr_pce_predict through the C ABI on a real MI355X, in both dtypes.  The truth is the definition in fp64 on
the CPU applied to the inputs as rounded to the dtype; the bound is entry-wise and derived (pce_cases.kernel_bound), with A the
same expression on absolute values:

    (2 S + N + C' + 4) 2^-52 A,  C' = 0 for the design matrix and C for predict;  in fp32 + 2^-23 |truth|, the rounding at the store

Shapes: every P of {1, 63, 64, 65, 257, 1000} against every C of {1, 19, 64, 65, 300} (below / at / above a wave and a tile of
points resp. candidates, more than one workgroup, a partial last tile) at (N, S) = (1, 1), (3, 4), (5, 3); S at its limit, N S at
its limit (N = 256 and 16 x 16: the smallest point tiles) at two of those (P, C); one step past each limit."""
import re

import numpy as np
import pytest
import torch

import pce_cases as pc
from tntorch_amd import _hip as h

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
SENTINEL = -77.0


def _within(out, truth, bound, what, worst):
    err = np.abs(out.cpu().double().numpy() - truth)
    worst[0], worst[1] = max(worst[0], float(err.max())), max(worst[1], float((err - bound).max()))
    assert bool((err <= bound).all()), (what, float(err.max()), float((err - bound).max()))


def _run_grid(N, S, dt, pairs):
    Z, Psi, coords, coef, M, A = pc.kernel_inputs(N, S, dt)
    Zd, Psid, cd, cfd = Z.cuda(), Psi.cuda(), coords.cuda(), coef.cuda()
    wd, wp = [0.0, -np.inf], [0.0, -np.inf]
    for P, C in pairs:
        what = "N {} S {} P {} C {} {}".format(N, S, P, C, dt)
        out, flag = h.pce_design(Zd[:P], Psid, cd[:C])
        assert out.is_cuda and out.dtype == dt and tuple(out.shape) == (P, C) and out.is_contiguous()
        _within(out, M[:P, :C], pc.kernel_bound(N, S, 0, dt, M[:P, :C], A[:P, :C]), "design " + what, wd)
        again, flag2 = h.pce_design(Zd[:P], Psid, cd[:C])
        assert torch.equal(out, again)                                       # bit-identical from call to call
        y, flag3 = h.pce_predict(Zd[:P], Psid, cd[:C], cfd[:C])
        assert y.is_cuda and y.dtype == dt and tuple(y.shape) == (P,)
        ty, Ay = pc.truth_predict(M, A, coef, P, C)
        _within(y, ty, pc.kernel_bound(N, S, C, dt, ty, Ay), "predict " + what, wp)
        assert torch.equal(y, h.pce_predict(Zd[:P], Psid, cd[:C], cfd[:C])[0])
        assert int(flag.item()) == 0 and int(flag2.item()) == 0 and int(flag3.item()) == 0
    print("N {} S {} {}: design largest error {:.3e} largest excess {:.3e}; predict largest error {:.3e} largest excess {:.3e}".format(
        N, S, dt, wd[0], wd[1], wp[0], wp[1]))
    assert torch.equal(Zd.cpu(), Z) and torch.equal(Psid.cpu(), Psi) and torch.equal(cd.cpu(), coords) and torch.equal(cfd.cpu(), coef)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N, S", pc.KERNEL_NS)
def test_grid_of_points_and_candidates(N, S, dt):
    _run_grid(N, S, dt, [(P, C) for P in pc.KERNEL_P for C in pc.KERNEL_C])


@pytest.mark.parametrize("dt", DTYPES)
def test_at_the_limits(dt):
    """S = ttr_pce_max_order() with two modes, and N S = ttr_pce_max_basis(): the largest N (S = 1) and the largest S."""
    so, nb = h.pce_max_order(), h.pce_max_basis()
    assert (so, nb) == (16, 256)
    for N, S in ((2, so), (nb, 1), (nb // so, so)):
        _run_grid(N, S, dt, pc.EXTRA_PC)


@pytest.mark.parametrize("dt", DTYPES)
def test_past_the_limits_nothing_is_launched(dt):
    L, code = h.lib(), h.dtype_code(dt)
    so, nb = h.pce_max_order(), h.pce_max_basis()
    P, C = 65, 19
    for N, S in ((1, so + 1), (nb + 1, 1), (nb // so + 1, so)):
        Z, Psi = torch.zeros(P, N, dtype=dt).cuda(), torch.zeros(N, S, S, dtype=dt).cuda()
        coords, coef = torch.zeros(C, N, dtype=torch.int64).cuda(), torch.ones(C, dtype=dt).cuda()
        M, y = torch.full((P, C), SENTINEL, dtype=dt).cuda(), torch.full((P,), SENTINEL, dtype=dt).cuda()
        flag = torch.zeros(1, dtype=torch.int32).cuda()
        assert L.ttr_pce_design(code, P, N, S, C, Z.data_ptr(), N, 1, Psi.data_ptr(), coords.data_ptr(), M.data_ptr(), C, flag.data_ptr(),
                                None) == h.E_INVALID
        assert L.ttr_pce_predict(code, P, N, S, C, Z.data_ptr(), N, 1, Psi.data_ptr(), coords.data_ptr(), coef.data_ptr(), y.data_ptr(),
                                 flag.data_ptr(), None) == h.E_INVALID
        with pytest.raises(ValueError):
            h.pce_design(Z, Psi, coords)
        with pytest.raises(ValueError):
            h.pce_predict(Z, Psi, coords, coef)
        torch.cuda.synchronize()
        assert bool((M.cpu() == SENTINEL).all()) and bool((y.cpu() == SENTINEL).all()) and int(flag.item()) == 0


@pytest.mark.parametrize("dt", DTYPES)
def test_strided_features_and_padded_output(dt):
    """Z as a column slice of a wider matrix and as a transposed view gives the bits of the contiguous Z; with ldm > C the
    padding of M keeps its sentinel."""
    N, S, P, C = 3, 4, 257, 65
    Z, Psi, coords, coef, M, A = pc.kernel_inputs(N, S, dt)
    Z = Z[:P]
    Psid, cd, cfd = Psi.cuda(), coords[:C].cuda(), coef[:C].cuda()
    ref, _ = h.pce_design(Z.cuda(), Psid, cd)
    yref, _ = h.pce_predict(Z.cuda(), Psid, cd, cfd)
    wide = torch.full((P, N + 4), 9.0, dtype=dt)
    wide[:, 2 : 2 + N] = Z
    sl = wide.cuda()[:, 2 : 2 + N]
    tr = Z.t().contiguous().cuda().t()
    assert sl.stride() == (N + 4, 1) and tr.stride() == (1, P)
    for view in (sl, tr):
        assert torch.equal(h.pce_design(view, Psid, cd)[0], ref) and torch.equal(h.pce_predict(view, Psid, cd, cfd)[0], yref)
    worst = [0.0, -np.inf]
    _within(ref, M[:P, :C], pc.kernel_bound(N, S, 0, dt, M[:P, :C], A[:P, :C]), "design", worst)
    big = torch.full((P, C + 7), SENTINEL, dtype=dt).cuda()
    got, _ = h.pce_design(Z.cuda(), Psid, cd, out=big[:, :C])
    assert got.data_ptr() == big.data_ptr() and torch.equal(big[:, :C], ref) and bool((big[:, C:].cpu() == SENTINEL).all())
    with pytest.raises(ValueError):
        h.pce_design(Z.cuda(), Psid, cd, out=torch.empty(C, P, dtype=dt).cuda().t())   # not contiguous along c


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("bad", [4, -1])
def test_a_coordinate_outside_the_basis_zeroes_its_candidate_and_sets_the_flag(bad, dt):
    N, S, P, C = 3, 4, 130, 70
    Z, Psi, coords, coef, _, _ = pc.kernel_inputs(N, S, dt)
    Zd, Psid, cfd = Z[:P].cuda(), Psi.cuda(), coef[:C].cuda()
    clean, flag = h.pce_design(Zd, Psid, coords[:C].cuda())
    yclean, _ = h.pce_predict(Zd, Psid, coords[:C].cuda(), cfd)
    assert int(flag.item()) == 0
    hit = 66
    c = coords[:C].clone()
    c[hit, 1] = bad
    got, flag = h.pce_design(Zd, Psid, c.cuda())
    assert int(flag.item()) == 1
    keep = torch.ones(C, dtype=torch.bool)
    keep[hit] = False
    assert torch.equal(got[:, keep], clean[:, keep]) and bool((got[:, hit] == 0).all())
    y, flag = h.pce_predict(Zd, Psid, c.cuda(), cfd)
    assert int(flag.item()) == 1
    cf0 = coef[:C].clone()
    cf0[hit] = 0.0        # the same sum with that term exactly zero
    assert torch.equal(y, h.pce_predict(Zd, Psid, coords[:C].cuda(), cf0.cuda())[0]) and not torch.equal(y, yclean)
    flag = torch.full((1,), 6, dtype=torch.int32).cuda()     # other bits of the flag are kept
    h.pce_design(Zd, Psid, c.cuda(), flag=flag)
    assert int(flag.item()) == 7


def test_symbols_are_declared_and_exported():
    with open(h._HEADER) as f:
        header = f.read()
    for name in ("ttr_pce_design", "ttr_pce_predict", "ttr_pce_max_order", "ttr_pce_max_basis"):
        assert re.search(r"\bint\s+{}\s*\(".format(name), header), name
        assert name in h.EXPORTED_SYMBOLS and hasattr(h.lib(), name)

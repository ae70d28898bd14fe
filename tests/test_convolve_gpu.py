"""``tn.convolve`` on device tensors (a real MI355X) against the dense fp64 truths of tests/golden/convolve_f64.npz with the host
bounds; in fp32 the derived bound of the exact path, N (n_max + 2) 2^-24 ||absconv train|| (convolve_cases.fp32_exact_bound), is
added.  Results live on the device in the input dtype, and agree with the CPU mirror's in ranks and shapes."""
import numpy as np
import pytest
import torch

import convolve_cases as cc
import tntorch_amd as tn

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64 = torch.float32, torch.float64


def _on_device(t, dt):
    assert isinstance(t, tn.Tensor) and all(U is None for U in t.Us)
    for c in t.cores:
        assert c.is_cuda and c.dtype == dt


@pytest.mark.parametrize("case", cc.cases())
def test_golden_fp64(case):
    t1, t2, mode = cc.operands(case, F64, DEV)
    exact = tn.convolve(t1, t2, mode=mode, eps=None)
    _on_device(exact, F64)
    err = cc.rel_err(cc.dense64(exact), cc.truth(case))
    print(case, "exact fp64: relative error", err)
    assert err <= 1e-12
    rounded = tn.convolve(t1, t2, mode=mode, eps=1e-6)
    _on_device(rounded, F64)
    err = cc.rel_err(cc.dense64(rounded), cc.truth(case))
    print(case, "eps = 1e-6 fp64: relative error", err, "ranks", rounded.ranks_tt.tolist())
    assert err <= 1e-6 + 1e-12


@pytest.mark.parametrize("case", cc.cases())
def test_golden_fp32(case):
    t1, t2, mode = cc.operands(case, F32, DEV)
    exact_bound = cc.fp32_exact_bound(t1, t2, mode, cc.truth(case))
    exact = tn.convolve(t1, t2, mode=mode, eps=None)
    _on_device(exact, F32)
    err = cc.rel_err(cc.dense64(exact), cc.truth(case))
    print(case, "exact fp32: relative error", err, "bound", exact_bound)
    assert err <= exact_bound
    rounded = tn.convolve(t1, t2, mode=mode, eps=1e-4)
    _on_device(rounded, F32)
    err = cc.rel_err(cc.dense64(rounded), cc.truth(case))
    print(case, "eps = 1e-4 fp32: relative error", err, "bound", 1e-4 + exact_bound)
    assert err <= 1e-4 + exact_bound


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("case", ["pq_full", "qp_same", "mn_valid", "kh_same", "pg_same", "vw_full"])
def test_ranks_and_shapes_equal_the_cpu_mirrors(case, dt):
    d1, d2, mode = cc.operands(case, dt, DEV)
    h1, h2, _ = cc.operands(case, dt)
    dev, host = tn.convolve(d1, d2, mode=mode, eps=None), tn.convolve(h1, h2, mode=mode, eps=None)
    assert dev.ranks_tt.tolist() == host.ranks_tt.tolist() and list(dev.shape) == list(host.shape)
    for x, y in zip(dev.cores, host.cores):
        assert tuple(x.shape) == tuple(y.shape)
    assert cc.rel_err(cc.dense64(dev), cc.dense64(host)) <= (1e-5 if dt == F32 else 1e-13)


def test_rank_one_kernel_keeps_the_ranks():
    t1, g, mode = cc.operands("pg_same", F32, DEV)
    out = tn.convolve(t1, g, mode=mode)
    _on_device(out, F32)
    assert out.ranks_tt.tolist() == t1.ranks_tt.tolist() and list(out.shape) == list(t1.shape)


@pytest.mark.parametrize("dt", [F32, F64])
def test_rmax_below_the_product_ranks(dt):
    """p * q has product ranks 6; rmax = 4 truncates.  Bound: twice the error that round_tt of the mirror's exact train gives on
    the CPU in the same dtype (rank-rule noise can pick a neighbouring rank); both figures are printed."""
    case = "pq_full"
    h1, h2, mode = cc.operands(case, dt)
    host = tn.Tensor([c.to(dt) for c in cc.mirror_train(h1, h2, mode)])
    host.round_tt(eps=0, rmax=4)
    bound = 2 * cc.rel_err(cc.dense64(host), cc.truth(case))
    d1, d2, _ = cc.operands(case, dt, DEV)
    out = tn.convolve(d1, d2, mode=mode, eps=None, rmax=4)
    _on_device(out, dt)
    assert max(out.ranks_tt.tolist()) == 4
    err = cc.rel_err(cc.dense64(out), cc.truth(case))
    print(dt, "rmax = 4: relative error", err, "bound (2 x the CPU's)", bound)
    assert 0 < bound and err <= bound


def test_refuses_different_devices_and_dtypes():
    d1, d2, _ = cc.operands("pq_full", F64, DEV)
    h1, h2, _ = cc.operands("pq_full", F64)
    with pytest.raises(ValueError):
        tn.convolve(d1, h2)
    with pytest.raises(ValueError):
        tn.convolve(h1, d2)
    with pytest.raises(ValueError):
        tn.convolve(d1, cc.train("q", F32, DEV))

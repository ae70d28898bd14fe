"""tntorch_amd/derivatives.py on device tensors (a real MI355X): the quantities of tests/golden/derivatives_f64.npz with the host
bounds in fp64, and in fp32 with the inputs cast (tests/derivatives_cases.py); results live on the device; device and host mirror
agree on the Laplacian's ranks and values."""
import numpy as np
import pytest
import torch

import derivatives_cases as dc
import tntorch_amd as tn

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64 = torch.float32, torch.float64


def _on_device(t, dt):
    assert isinstance(t, tn.Tensor)
    for c in t.cores:
        assert c.is_cuda and c.dtype == dt
    for U in t.Us:
        assert U is None or (U.is_cuda and U.dtype == dt)


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("q", sorted(dc.TENSOR))
def test_tensor_valued_golden(q, dt):
    out = dc.TENSOR[q](tn, dt, DEV)
    _on_device(out, dt)
    dc.check_tensor(q, out, dt)   # 5e-6 (fp32) / 1e-12 (fp64) of the largest entry of the truth


def test_sensitivity_fp64():
    nu = dc.dgsm(tn, F64, DEV)
    assert nu.is_cuda and nu.dtype == F64 and nu.shape == (4,)
    assert dc.rel_err(nu, "dgsm_a") < 1e-10
    assert dc.rel_err(nu, "dgsm_a", against=dc.ref("dgsm_a")) < 1e-5
    M = dc.as_matrix(tn, F64, DEV)
    assert M.is_cuda and dc.rel_err(M, "as_M") < 1e-10
    w, v = dc.active_subspace(tn, F64, DEV)
    assert w.is_cuda and v.is_cuda and w.dtype == F64 and v.dtype == F64
    assert dc.rel_err(w, "as_w") < 1e-10 and dc.rel_err(w, "as_w", against=dc.ref("as_w")) < 1e-5
    assert dc.rel_err(dc.align_signs(v), "as_v") < 1e-10


def test_sensitivity_fp32():
    """The bound is four times the error of the host mirror in fp32 on the same inputs against the truth, with a floor of 1e-6
    (relative to the largest entry of the truth).  Observed on the host: the mirror's fp32 error is 1.25e-7 (dgsm) and 1.38e-7
    (M), so the floor decides: both bounds are 1e-6, eight fp32 roundings.  The device's figures are printed by the test."""
    bounds = {}
    for q, call in (("dgsm_a", dc.dgsm), ("as_M", dc.as_matrix)):
        host = dc.rel_err(call(tn, F32, "cpu"), q)
        bounds[q] = max(4.0 * host, 1e-6)
        out = call(tn, F32, DEV)
        assert out.is_cuda and out.dtype == F32
        err = dc.rel_err(out, q)
        print(q, "fp32: host mirror error", host, "bound", bounds[q], "device error", err)
        assert err <= bounds[q], (q, err, bounds[q])
    # the eigenpairs of an M within bounds["as_M"]: |dw| <= ||dM||_2 <= N max|dM| and max|M| <= w_0, so N times the bound of M
    # relative to w_0; eigenvectors move by at most ||dM||_2 over the smallest gap (Davis-Kahan, to first order); plus one fp32
    # rounding of the fp64 eigenpairs (1e-6 with room)
    w, v = dc.active_subspace(tn, F32, DEV)
    assert w.is_cuda and v.is_cuda and w.dtype == F32 and v.dtype == F32
    tw = dc.truth("as_w")
    gap = float(np.abs(np.diff(tw)).min() / tw[0])
    bw, bv = 4 * bounds["as_M"] + 1e-6, 4 * bounds["as_M"] / gap + 1e-6
    ew, ev = dc.rel_err(w, "as_w"), dc.rel_err(dc.align_signs(v), "as_v")
    print("as_w fp32: bound", bw, "device error", ew, " as_v: bound", bv, "device error", ev)
    assert ew <= bw and ev <= bv


def test_dgsm_returns_a_device_tensor_without_reading_it():
    """As for the moments: the result is a tensor on the device in the input's dtype -- nothing on the way reads a value back
    (a host read inside would be a ``.item()`` / ``float()`` on an interface, and the result would not need to be a device tensor)."""
    for dt in (F32, F64):
        nu = tn.dgsm(dc.train("a", dt, DEV), dc.bounds("a"), dc.marginals(dt, DEV))
        assert isinstance(nu, torch.Tensor) and nu.is_cuda and nu.dim() == 1 and nu.dtype == dt
        nu0 = tn.dgsm(dc.train("a", dt, DEV), dc.bounds("a"))   # default marginals are created on the device
        assert nu0.is_cuda and nu0.dtype == dt


def test_device_and_host_agree_on_the_laplacian():
    for name in ("a", "f0", "k", "v"):
        b = dc.bounds("f" if name == "f0" else name)
        for dt, bound in ((F32, 5e-6), (F64, 1e-12)):
            d = tn.laplacian(dc.train(name, dt, DEV), bounds=b)
            c = tn.laplacian(dc.train(name, dt, "cpu"), bounds=b)
            _on_device(d, dt)
            assert d.ranks_tt.tolist() == c.ranks_tt.tolist()
            scale = float(np.abs(dc.truth("laplacian_" + name)).max())
            for cd, cc in zip(d.cores, c.cores):
                assert cd.shape == cc.shape
            assert float((d.torch().cpu() - c.torch()).abs().max()) <= 2 * bound * scale   # each side within `bound` of the truth
    t = dc.train("a", F64, DEV)
    lap = tn.laplacian(t, bounds=dc.bounds("a"))
    assert lap.ranks_tt.tolist() == [1, 6, 6, 6, 1]
    rounded = lap.clone()
    rounded.round_tt(eps=1e-10)   # the consumer: the structured train goes straight into round_tt
    assert dc.rel_err(rounded.torch(), "laplacian_a") < 1e-8


def test_partial_keeps_tucker_factors_on_device():
    k = dc.train("k", F64, DEV)
    out = tn.partial(k, 0, order=3, bounds=dc.bounds("k")[0], periodic=True)
    assert out.Us[0] is not None and out.Us[0].is_cuda and torch.equal(out.cores[0], k.cores[0])
    dc.check_tensor("partial_k_d0_o3_p1", out, F64)
    big = tn.partial(dc.train("a", F64, DEV), 1, order=6, bounds=dc.bounds("a")[1])   # above the fused limit: chained launches
    ref = tn.partial(dc.train("a", F64, "cpu"), 1, order=6, bounds=dc.bounds("a")[1])
    r = ref.torch()
    assert float((big.torch().cpu() - r).abs().max()) < 1e-12 * float(r.abs().max())

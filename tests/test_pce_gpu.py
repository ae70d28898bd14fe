"""``PCEInterpolator`` end to end on device tensors (a real MI355X), in both dtypes: the exact-recovery problem and a noisy one
(P = 300, N = 3, p = 4) against the CPU mirror on the same data."""
import pytest
import torch

import pce_cases as pc
import tntorch_amd as tn
from tntorch_amd import _hip

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]


def _fit(X, y, **kw):
    m = tn.PCEInterpolator()
    m.fit(X, y, verbose=False, **kw)
    return m


def _problem(name):
    return pc.recovery_problem() if name == "recovery" else pc.noisy_problem(300, 3)


@pytest.fixture(scope="module")
def mirrors():
    """The CPU mirror's fp64 fit of both problems, computed once."""
    out = {}
    for name in ("recovery", "noisy"):
        X, y = _problem(name)
        out[name] = (X, y, _fit(X, y, p=4))
    return out


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", ["recovery", "noisy"])
def test_fit_predict_to_tensor_on_the_device(name, dt, mirrors, monkeypatch):
    X, y, cpu = mirrors[name]
    Xd, yd = X.to(dt).cuda(), y.to(dt).cuda()
    m = _fit(Xd, yd, p=4)
    for t in (m.X_mean, m.X_std, m.Psis, m.coef, m.allcoef):
        assert t.is_cuda and t.dtype == dt
    assert m.coords.is_cuda and m.allcoords.is_cuda and m.coords.dtype == torch.int64
    assert torch.equal(m.allcoords.cpu(), cpu.allcoords)
    if dt == torch.float64:
        assert torch.equal(m.coords.cpu(), cpu.coords)          # the same selection as the CPU mirror's, in the same order
        print(name, "fp64 device coef against the CPU mirror's", pc.rel(m.coef, cpu.coef))

    def no_sync(*a, **k):
        raise AssertionError("predict synchronised with the device")

    from tntorch_amd import _hipops

    with monkeypatch.context() as mp:    # neither an explicit synchronise nor the read-back of the kernel's flag
        mp.setattr(torch.cuda, "synchronize", no_sync)
        mp.setattr(_hipops, "_pce_raise", no_sync)
        pred = m.predict(Xd)
    assert pred.is_cuda and pred.dtype == dt and tuple(pred.shape) == (X.shape[0],)
    dev = pc.rel(pred, cpu.predict(X))
    print(name, dt, "device predict against the CPU mirror's fp64 one", dev, "selected", int(m.coords.shape[0]))
    assert dev <= (pc.GPU_F32_PREDICT_CAP if dt == torch.float32 else 1e-9)
    if name == "recovery":
        err = pc.rel(pred, y)
        print("exact recovery on the device", dt, err)
        assert err <= (pc.RECOVERY_TOL if dt == torch.float64 else pc.GPU_F32_PREDICT_CAP)

    eps = 1e-10 if dt == torch.float64 else 1e-6
    t = m.to_tensor(domain=16, eps=eps, verbose=False)
    assert all(c.is_cuda and c.dtype == dt for c in t.cores) and all(U is not None and U.is_cuda and U.dtype == dt for U in t.Us)
    assert list(t.shape) == [16, 16, 16]
    onto = m.predict(pc.grid_points(m.bbox, 16, dt, device="cuda"))
    err = float(torch.norm(t.torch().reshape(-1).double() - onto.double()) / torch.norm(onto.double()))
    print(name, dt, "to_tensor against predict on the 16^3 grid", err)
    # fp32: the device TT-SVD takes its singular vectors from the Gram matrix of the unfolding, which resolves them to
    # sqrt(2^-24) = 2^-12 at best; that, not eps = 1e-6, bounds the agreement
    assert err <= (pc.TENSOR_TOL if dt == torch.float64 else 2.0 ** -12)


def test_device_limits_and_bad_coordinates_raise_value_error():
    from tntorch_amd import _hipops

    X, y = pc.recovery_problem()
    with pytest.raises(ValueError, match="device limits"):
        tn.PCEInterpolator().fit(X.cuda(), y.cuda(), p=_hip.pce_max_order() + 1, verbose=False)
    wide = torch.rand(200, _hip.pce_max_basis() // 4 + 1, dtype=torch.float64).cuda()     # N * ceil(p) = 260 > 256
    with pytest.raises(ValueError, match="device limits"):
        tn.PCEInterpolator().fit(wide, y[:200].cuda(), p=4, verbose=False)
    Z, Psi, coords, coef, _, _ = pc.kernel_inputs(3, 4, torch.float64)
    c = coords[:10].clone()
    c[3, 0] = 4
    with pytest.raises(ValueError, match="outside"):
        _hipops.pce_design(Z[:20].cuda(), Psi.cuda(), c.cuda())
    with pytest.raises(ValueError, match="outside"):
        _hipops.pce_predict(Z[:20].cuda(), Psi.cuda(), c.cuda(), coef[:10].cuda())
    assert _hipops.pce_predict(Z[:20].cuda(), Psi.cuda(), c.cuda(), coef[:10].cuda(), check=False).shape == (20,)

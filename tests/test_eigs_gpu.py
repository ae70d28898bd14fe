"""``tn.tt_eigsh`` on device tensors: the cases of ``test_eigs_host.py`` with the same recorded bounds
(``eigs_cases.MEASURED_*``, 4 x the host mirror's worst case), the host mirror's value from the same start, and one problem whose
local vectors span several workgroups."""
import math

import pytest
import torch

import eigs_cases as ec
import solve_cases as sc
import tntorch_amd as tn
from tntorch_amd import tteigs

pytestmark = pytest.mark.gpu

DTYPES = ec.DTYPES


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("which", ec.WHICH)
@pytest.mark.parametrize("name, ranks", ec.checked_cases())
def test_value_and_residual(name, ranks, which, dt):
    A = ec.matrix(name, dt, "cuda")
    x0 = ec.start(name, dt, ranks, seed=0, device="cuda")
    before = dict(tteigs.READBACKS)
    value, x, info = tn.tt_eigsh(A, x0=x0, which=which, tol=ec.TOL[dt], return_info=True)
    assert tteigs.READBACKS["sweep"] - before["sweep"] == info["sweeps"] and tteigs.READBACKS["residual"] - before["residual"] == 1
    assert value.is_cuda and value.dim() == 0 and value.dtype == dt and not value.requires_grad
    assert all(c.is_cuda and c.dtype == dt and not c.requires_grad and c.grad_fn is None for c in x.cores)
    err, res = ec.value_error(name, dt, which, value), ec.dense_residual(name, dt, value, x)
    host_value, _ = tn.tt_eigsh(ec.matrix(name, dt), x0=ec.start(name, dt, ranks, seed=0), which=which, tol=ec.TOL[dt])
    print("{} ranks {} {} {}: {} sweeps, value error {:.3e}, dense residual {:.3e}, device - host {:.3e}".format(
        name, ranks, which, dt, info["sweeps"], err, res, float(value) - float(host_value)))
    assert info["converged"] and info["sweeps"] == 2
    assert err <= ec.value_bound(dt)
    assert res <= ec.residual_bound(dt) and res <= ec.tol_of(dt)
    assert abs(float(value) - float(host_value)) <= ec.value_bound(dt) * abs(float(host_value))
    assert abs(info["residual"] - res) <= 0.05 * res + 64 * ec.unit(dt)
    assert abs(float(ec.dense(x).norm()) - 1.0) <= 16 * len(ec.MATRICES[name][1]) * ec.eps(dt)
    assert [int(r) for r in x.ranks_tt] == [int(r) for r in x0.ranks_tt]


def test_grad_operands():
    dt = torch.float64
    A = ec.matrix("laplace", dt, "cuda")
    x0 = ec.start("laplace", dt, 1, device="cuda")
    A.cores[1].requires_grad_(True)
    with pytest.raises(NotImplementedError, match="not differentiable on the device"):
        tn.tt_eigsh(A, x0=x0, tol=1e-9)
    with torch.no_grad():
        value, x = tn.tt_eigsh(A, x0=x0, tol=1e-9)
    assert not value.requires_grad and all(not c.requires_grad for c in x.cores)
    assert ec.value_error("laplace", dt, "SA", value) <= ec.value_bound(dt)
    A.cores[1].requires_grad_(False)
    x0.cores[0].requires_grad_(True)
    with pytest.raises(NotImplementedError, match="not differentiable on the device"):
        tn.tt_eigsh(A, x0=x0, tol=1e-9)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("which", ec.WHICH)
def test_sixteen_to_the_fourth(which, dt):
    """shift I + c sum_k L_k on [16]^4 at ranks 8: a local vector has up to 8 * 16 * 8 = 1024 elements (more than one pack per
    thread of a workgroup in fp64, a 64-wide tile of the matvec).  The extreme eigenvector has rank 1, so the value meets the
    bound of the small cases; the truth is the closed form shift + c sum_k (2 -+ 2 cos(pi / (n_k + 1)))."""
    dims, shift, c = [16] * 4, 1.0, 0.25
    G = [g.to(dt) for g in sc.laplace_cores(dims, shift=shift, c=c)]
    A = tn.TTMatrix([g.cuda() for g in G], None, dims, dims)
    sign = -1.0 if which == "SA" else 1.0
    truth = shift + c * sum(2.0 + sign * 2.0 * math.cos(math.pi / (n + 1)) for n in dims)
    torch.manual_seed(0)
    value, x, info = tn.tt_eigsh(A, ranks_tt=8, which=which, tol=ec.TOL[dt], return_info=True)
    err = abs(float(value) - truth) / abs(truth)
    print("[16]^4 ranks 8 {} {}: {} sweeps, value error {:.3e}, residual {:.3e}".format(which, dt, info["sweeps"], err, info["residual"]))
    assert info["converged"] and [int(r) for r in x.ranks_tt] == [1, 8, 8, 8, 1]
    assert err <= ec.value_bound(dt)
    assert info["residual"] <= ec.residual_bound(dt) and info["residual"] <= ec.tol_of(dt)

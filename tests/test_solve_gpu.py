"""``tn.tt_solve`` on a real MI355X: the cases and conditions of test_solve_host.py with device operands (dense residual <= tol,
error <= cond(A) tol, monotone energy; every truth dense fp64 on the CPU), the agreement with the CPU mirror, and the driver's
contract: one readback per sweep, results on the device, the grad refusal."""
import pytest
import torch

import solve_cases as sc
import tntorch_amd as tn
from tntorch_amd import ttsolve

pytestmark = pytest.mark.gpu

DTYPES = sc.DTYPES
TOL, tol_of, build, dense, rel_residual = sc.TOL, sc.tol_of, sc.build, sc.dense, sc.rel_residual


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(sc.MATRICES))
def test_full_ranks_solve_in_one_sweep(name, dt):
    A, b, D, bd, xd, cond = build(name, "random", dt, "cuda")
    tol = tol_of(dt)
    x1 = tn.tt_solve(A, b, ranks_tt=sc.FULL_RANKS[name], nswp=1, tol=TOL[dt])
    res = rel_residual(D, bd, x1)
    print("full ranks {} {}: dense residual after one sweep {:.3e}".format(name, dt, res))
    assert res <= tol
    x, info = tn.tt_solve(A, b, ranks_tt=99, tol=TOL[dt], return_info=True)
    assert info["converged"] and info["sweeps"] == 2
    assert all(c.is_cuda and c.dtype == dt and not c.requires_grad for c in x.cores)
    res = rel_residual(D, bd, x)
    assert res <= tol and abs(info["residual"] - res) <= 0.05 * res + 64 * sc.unit(dt)
    assert float((dense(x) - xd).norm() / xd.norm()) <= cond * tol


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("name", ["laplace", "laplace4", "shifted"])
def test_rank_two_systems(name, seed, dt):
    """As on the host: convergence within 20 sweeps, residual, error and the monotone energy; and from the same x0 the device and
    the CPU mirror stop after the same number of sweeps, give or take one, with solutions 2 cond(A) tol apart at most."""
    A, b, D, bd, xd, cond = build(name, "product", dt, "cuda")
    tol, dims = tol_of(dt), sc.MATRICES[name][1]
    start = [c.to(dt) for c in sc.start_cores(dims, seed)]
    x0 = tn.Tensor([c.cuda() for c in start])
    keep = [c.clone() for c in x0.cores]
    before = dict(ttsolve.READBACKS)
    x, info = tn.tt_solve(A, b, x0=x0, tol=TOL[dt], return_info=True)
    assert ttsolve.READBACKS["sweep"] - before["sweep"] == info["sweeps"]          # one readback per sweep
    assert ttsolve.READBACKS["setup"] - before["setup"] == 1 and ttsolve.READBACKS["residual"] - before["residual"] == 1
    assert all(torch.equal(a, c) for a, c in zip(keep, x0.cores))
    assert info["converged"] and info["sweeps"] <= 20
    res = rel_residual(D, bd, x)
    err = float((dense(x) - xd).norm() / xd.norm())
    print("rank 2 {} seed {} {}: {} sweeps, dense residual {:.3e}, error {:.3e}".format(name, seed, dt, info["sweeps"], res, err))
    assert res <= tol and err <= cond * tol
    energies = [sc.energy(D, bd, dense(x0))]
    for s in range(1, info["sweeps"] + 1):
        energies.append(sc.energy(D, bd, dense(tn.tt_solve(A, b, x0=x0, nswp=s, tol=TOL[dt]))))
    for e0, e1 in zip(energies, energies[1:]):
        assert e1 <= e0 + 8 * sc.unit(dt) * abs(e0), energies
    if dt == torch.float64:
        Ac, bcpu, *_ = build(name, "product", dt, "cpu")
        xc, ic = tn.tt_solve(Ac, bcpu, x0=tn.Tensor(start), tol=TOL[dt], return_info=True)
        assert abs(ic["sweeps"] - info["sweeps"]) <= 1
        assert float((dense(x) - dense(xc)).norm() / xd.norm()) <= 2 * cond * tol


@pytest.mark.parametrize("dt", DTYPES)
def test_transpose_zero_and_single_mode(dt):
    A, b, D, bd, xd, cond = build("laplace", "random", dt, "cuda")
    xt = tn.tt_solve(A, b, transpose=True, ranks_tt=[4, 5], tol=TOL[dt])
    assert rel_residual(D, bd, xt) <= tol_of(dt) and xt.cores[0].is_cuda
    z = tn.tt_solve(A, tn.Tensor([torch.zeros_like(c) for c in b.cores]), ranks_tt=2)
    assert all(c.is_cuda and c.dtype == dt for c in z.cores) and float(z.torch().abs().max()) == 0.0
    G1 = sc.laplace_cores([6])
    b1 = torch.arange(1, 7, dtype=dt)
    x1, info = tn.tt_solve(tn.TTMatrix([G1[0].to(dt).cuda()], None, [6], [6]), tn.Tensor([b1[None, :, None].cuda()]), ranks_tt=1,
                           tol=TOL[dt], return_info=True)
    assert info["converged"]
    assert float((G1[0][0, :, :, 0] @ x1.torch().cpu().double() - b1.double()).norm() / b1.double().norm()) <= tol_of(dt)


def test_an_indefinite_matrix_is_refused_on_the_device():
    dims = [4, 3, 5]
    G = [g.cuda() for g in sc.laplace_cores(dims, shift=-2.0)]
    b = tn.Tensor([c.cuda() for c in sc.train_cores(dims, [2, 2], 31)])
    with pytest.raises(ValueError, match="not positive definite"):
        tn.tt_solve(tn.TTMatrix(G, None, dims, dims), b, ranks_tt=[4, 5], tol=1e-9)


def test_grad_operands_on_the_device():
    dt = torch.float64
    A, b, D, bd, xd, cond = build("laplace", "product", dt, "cuda")
    b.cores[1].requires_grad_(True)
    with pytest.raises(NotImplementedError, match="tt_solve is not differentiable on the device"):
        tn.tt_solve(A, b, ranks_tt=2)
    with torch.no_grad():
        x = tn.tt_solve(A, b, ranks_tt=2, tol=1e-9)
    assert all(c.is_cuda and not c.requires_grad for c in x.cores) and rel_residual(D, bd, x) <= 1e-9
    b.cores[1].requires_grad_(False)
    A.cores[0].requires_grad_(True)
    with pytest.raises(NotImplementedError, match="tt_solve is not differentiable on the device"):
        tn.tt_solve(A, b, ranks_tt=2)

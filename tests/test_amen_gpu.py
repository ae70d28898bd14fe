"""``tn.tt_amen_solve`` on a real MI355X: the convergence cases of test_amen_host.py at kickrank 2 with device operands and the same
bounds (every truth dense fp64 on the CPU), the ranks of every sweep against the CPU mirror's, strided matrix cores, and the
grad refusal.

The ranks are pinned on ``kron`` and ``shifted`` only: there every truncation of the host run lies at least 0.39 delta away from
its threshold in both dtypes (measured on the CPU: the distance of the nearest tail norm of the singular values from delta), six
orders of magnitude more than the ``100 u`` a rounding difference between the two devices could move it."""
import pytest
import torch

import amen_cases as ac
import solve_cases as sc
import tntorch_amd as tn
from tntorch_amd import ttamen

pytestmark = pytest.mark.gpu

DTYPES = sc.DTYPES


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name,rhs", ac.SYSTEMS)
def test_converges_from_rank_one(name, rhs, dt):
    A, b, D, bd, _, cond = sc.build(name, rhs, dt, "cuda")
    tol = sc.tol_of(dt)
    before = dict(ttamen.READBACKS)
    x, info = tn.tt_amen_solve(A, b, kickrank=2, tol=tol, return_info=True)
    delta = {k: ttamen.READBACKS[k] - before[k] for k in before}
    assert delta == {"setup": 1, "sweep": info["sweeps"], "residual": 1, "round": 1}
    assert all(c.is_cuda and c.dtype == dt and not c.requires_grad for c in x.cores)
    res = ac.check_solution(name, rhs, 2, x, info, D, bd, cond, tol)
    assert abs(info["residual"] - res) <= 0.05 * res + 64 * sc.unit(dt)
    if name in ("kron", "shifted"):
        Ac, bcpu, *_ = sc.build(name, rhs, dt, "cpu")
        _, host = tn.tt_amen_solve(Ac, bcpu, kickrank=2, tol=tol, return_info=True)
        assert info["ranks"] == host["ranks"] and info["sweeps"] == host["sweeps"]


@pytest.mark.parametrize("dt", DTYPES)
def test_strided_matrix_cores(dt):
    """``tt_transpose`` views of the cores of the (symmetric) matrix: read where they lie, the default's residual bound."""
    A, b, D, bd, _, cond = sc.build("laplace", "random", dt, "cuda")
    At = tn.tt_transpose(A)
    assert any(not c.is_contiguous() for c in At.cores)
    tol = sc.tol_of(dt)
    for kw in (dict(), dict(transpose=True)):
        x, info = tn.tt_amen_solve(At, b, tol=tol, return_info=True, **kw)
        assert info["converged"] and sc.rel_residual(D, bd, x) <= ac.residual_bound(cond, tol)


@pytest.mark.parametrize("dt", DTYPES)
def test_start_train_and_rank_cap_on_the_device(dt):
    """``x0`` on the device is never written; ``rmax=3`` caps every rank of every sweep and of the returned train."""
    A, b, D, bd, _, cond = sc.build("laplace", "random", dt, "cuda")
    tol, dims = sc.tol_of(dt), sc.MATRICES["laplace"][1]
    x0 = tn.Tensor([c.to(dt).cuda() for c in sc.start_cores(dims, 1)])
    keep = [c.clone() for c in x0.cores]
    x, info = tn.tt_amen_solve(A, b, x0=x0, tol=tol, return_info=True)
    assert all(torch.equal(a, c) for a, c in zip(keep, x0.cores))
    assert info["converged"] and sc.rel_residual(D, bd, x) <= ac.residual_bound(cond, tol)
    x, info = tn.tt_amen_solve(A, b, rmax=3, tol=tol, nswp=3, return_info=True)
    assert all(r <= 3 for ranks in info["ranks"] for r in ranks) and all(int(r) <= 3 for r in x.ranks_tt)
    assert all(c.is_cuda for c in x.cores)


def test_grad_operands_on_the_device():
    dt = torch.float64
    A, b, D, bd, _, cond = sc.build("laplace", "product", dt, "cuda")
    b.cores[1].requires_grad_(True)
    with pytest.raises(NotImplementedError, match="tt_amen_solve is not differentiable on the device"):
        tn.tt_amen_solve(A, b)
    with torch.no_grad():
        x = tn.tt_amen_solve(A, b, tol=1e-9)
    assert all(c.is_cuda and not c.requires_grad for c in x.cores)
    assert sc.rel_residual(D, bd, x) <= ac.residual_bound(cond, 1e-9)
    b.cores[1].requires_grad_(False)
    A.cores[0].requires_grad_(True)
    with pytest.raises(NotImplementedError, match="tt_amen_solve is not differentiable on the device"):
        tn.tt_amen_solve(A, b)
    A.cores[0].requires_grad_(False)


def test_an_indefinite_matrix_is_refused_on_the_device():
    dims = [4, 3, 5]
    G = [g.cuda() for g in sc.laplace_cores(dims, shift=-2.0)]
    b = tn.Tensor([c.cuda() for c in sc.train_cores(dims, [2, 2], 31)])
    with pytest.raises(ValueError, match="not positive definite"):
        tn.tt_amen_solve(tn.TTMatrix(G, None, dims, dims), b, tol=1e-9)

"""``tn.optimize`` / ``tn.dof`` (autodiff.py:10-121) on CPU tensors, the host mirror of ttr_gather_grad, the grouping plan, and the
declarations of the new entry points."""
import math
import os
import re

import pytest
import torch

import tntorch_amd as tn
from tntorch_amd import _hip, _hostops, autodiff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def sgd(params):
    return torch.optim.SGD(params, lr=0.1)


def rank2_train(seed, requires_grad=False):
    g = torch.Generator().manual_seed(seed)
    rs = [1, 2, 2, 1]
    return tn.Tensor([torch.randn(rs[n], 4, rs[n + 1], generator=g, dtype=F64) for n in range(3)], requires_grad=requires_grad)


def test_exports_and_declarations():
    assert tn.optimize is tn.autodiff.optimize and tn.dof is tn.autodiff.dof
    assert tn.autodiff.__all__ == ["optimize", "dof"]
    header = open(os.path.join(ROOT, "include", "ttround_hip.h")).read()
    for name in ("ttr_gather_grad", "ttr_gather_grad_workspace_bytes", "ttr_gather_grad_stage_rows"):
        assert re.search(r"\b{}\s*\(".format(name), header) and name in _hip.EXPORTED_SYMBOLS
    assert "ttr_gather_grad" in header.split("#define TTR_ABI_VERSION")[0]  # named in the "ADDED under 17" list
    assert _hip.ABI_VERSION == 17
    makefile = open(os.path.join(ROOT, "tntorch_amd", "csrc", "Makefile")).read()
    assert re.search(r"^\s+ttr_autodiff\.hip\b", makefile, re.M)


def test_dof_counts_the_nodes_that_require_grad():
    g = torch.Generator().manual_seed(0)
    cores = [torch.randn(1, 3, 2, generator=g), torch.randn(2, 5, 4, generator=g), torch.randn(4, 6, 1, generator=g)]
    Us = [None, torch.randn(7, 5, generator=g), torch.randn(8, 6, generator=g)]
    t = tn.Tensor(cores, Us=Us)
    assert tn.dof(t) == 0
    cores[1].requires_grad_()
    Us[2].requires_grad_()
    assert tn.dof(t) == 2 * 5 * 4 + 8 * 6
    assert tn.dof(tn.Tensor(cores, Us=Us, requires_grad=True)) == 6 + 40 + 24 + 35 + 48


def reference_stop(x0sq, tol):
    """The iteration at which autodiff.py:67-78 stops for the losses l_k = x0sq * 0.64^k of SGD(lr = 0.1) on sum(x^2)."""
    l = [x0sq * 0.64 ** k for k in range(200)]
    for k in range(2, 200):
        if (l[k] <= tol or (l[k - 1] - l[k]) / l[k] <= tol) and l[k - 1] - l[k] < l[k - 2] - l[k - 1]:
            return k
    raise AssertionError


def test_optimize_trajectory_and_stopping_rule(capsys):
    x0 = torch.tensor([1.0, -2.0, 0.5], dtype=F64)
    x = x0.clone().requires_grad_()
    seen = []

    def loss(v):
        seen.append(v.detach().clone())
        return (v ** 2).sum()

    tn.optimize(x, loss, optimizer=sgd, tol=1e-4, print_freq=10)
    stop = reference_stop(float((x0 ** 2).sum()), 1e-4)
    assert stop == math.ceil(math.log(1e-4 / 5.25) / math.log(0.64))  # l_k <= tol is what fires: (l_{k-1} - l_k) / l_k = 0.5625
    assert len(seen) == stop + 1
    for k, v in enumerate(seen):
        assert torch.allclose(v, x0 * 0.8 ** k, rtol=1e-12, atol=0)
    assert torch.allclose(x.detach(), x0 * 0.8 ** (stop + 1), rtol=1e-12, atol=0)
    lines = capsys.readouterr().out.splitlines()
    masked = [re.sub(r"total time:\s+\d+\.\d{4}", "total time: T", s) for s in lines]
    assert len(masked) == stop // 10 + 2
    for j, s in enumerate(masked[:-1]):
        k = 10 * j
        assert s == "iter: {: <7} | loss: {:10.6f} | total time: T".format(k, 5.25 * 0.64 ** k), s
    assert masked[-1] == "iter: {: <7} | loss: {:10.6f} | total time: T <- converged (tol=0.0001)".format(stop, 5.25 * 0.64 ** stop)


def test_optimize_max_iter_and_loss_tuples(capsys):
    x = torch.tensor([3.0], dtype=F64, requires_grad=True)
    calls = []

    def loss(v):
        calls.append(1)
        return (v ** 2).sum(), (0 * v).sum() + 1.0

    tn.optimize([x], loss, optimizer=sgd, tol=None, max_iter=7, print_freq=4)
    assert len(calls) == 8 and torch.allclose(x.detach(), torch.tensor([3.0 * 0.8 ** 8], dtype=F64))
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 3
    assert re.fullmatch(r"iter: 0 \| loss:   9\.000000 \+   1\.000000 =       10\.0 \| total time:\s+\d+\.\d{4}", out[0]), out[0]
    assert re.fullmatch(r"iter: 4 \| loss: .* \| total time:\s+\d+\.\d{4}", out[1])
    assert re.fullmatch(r"iter: 7 \| loss: .* \| total time:\s+\d+\.\d{4} <- max_iter was reached: 7", out[2]), out[2]
    tn.optimize(x, lambda v: (v ** 2).sum(), optimizer=sgd, max_iter=3, verbose=False)
    assert capsys.readouterr().out == ""


def test_optimize_value_errors():
    t = rank2_train(0)
    with pytest.raises(ValueError, match="no parameters"):
        tn.optimize(t, lambda t: tn.norm(t))
    with pytest.raises(ValueError, match="no parameters"):
        tn.optimize(torch.zeros(3), lambda v: v.sum())
    b = tn.Tensor([torch.randn(2, 1, 3, 2, requires_grad=True), torch.randn(2, 2, 3, 1, requires_grad=True)], batch=True)
    with pytest.raises(ValueError, match="Batched"):
        tn.optimize(b, lambda t: t.cores[0].sum())


def all_points():
    return torch.cartesian_prod(*[torch.arange(4)] * 3)


def test_cpu_fit_of_a_rank2_train():
    X = all_points()
    y = rank2_train(1)[X].torch()
    t = rank2_train(2, requires_grad=True)
    start = float(tn.relative_error(y, t[X]).detach())
    tn.optimize(t, lambda t: tn.relative_error(y, t[X]), max_iter=150, verbose=False)
    end = float(tn.relative_error(y, t[X]).detach())
    assert end < start and all(bool(torch.isfinite(c).all()) for c in t.cores)
    assert tn.dof(t) == 8 + 16 + 8 and all(c.grad is not None for c in t.cores)


def interfaces(cores, X):
    """Left interfaces L_n [P, r_n] and right interfaces R_n [P, r_{n+1}] for upstream gradient 1 on a [P] output."""
    P, N = X.shape[0], len(cores)
    Ls = [torch.ones(P, 1, dtype=F64)]
    for n in range(N - 1):
        Ls.append(torch.einsum("pa,apb->pb", Ls[-1], cores[n][:, X[:, n], :]))
    Rs = [torch.ones(P, 1, dtype=F64)]
    for n in range(N - 1, 0, -1):
        Rs.insert(0, torch.einsum("apb,pb->pa", cores[n][:, X[:, n], :], Rs[0]))
    return Ls, Rs


@pytest.mark.parametrize("task_samples", [None, 3])
def test_host_gather_grad_agrees_with_autograd(task_samples):
    t = rank2_train(3, requires_grad=True)
    X = all_points()[torch.randperm(64, generator=torch.Generator().manual_seed(4))[:50]]
    t[X].torch().sum().backward()
    cores = [c.detach() for c in t.cores]
    Ls, Rs = interfaces(cores, X)
    for n in range(3):
        col = X[:, n]
        perm = torch.sort(col, stable=True).indices
        plan = _hostops.GradPlan(torch.bincount(col, minlength=4).tolist(), "cpu", task_samples)
        dG = _hostops.gather_grad(Ls[n], Rs[n], perm, plan)
        assert torch.allclose(dG, t.cores[n].grad, rtol=1e-12, atol=1e-13)


def check_plan(counts, task_samples):
    plan = _hostops.GradPlan(counts, "cpu", task_samples)
    tb, te, toff = plan.tb.tolist(), plan.te.tolist(), plan.toff.tolist()
    assert len(toff) == len(counts) + 1 and toff[0] == 0 and toff[-1] == plan.ntasks == len(tb) == len(te)
    start = 0
    for i, n in enumerate(counts):  # the tasks of slice i tile its run [start, start + n) of the grouped samples, in order
        pos = start
        for t in range(toff[i], toff[i + 1]):
            assert tb[t] == pos and te[t] >= tb[t] and te[t] - tb[t] <= task_samples
            pos = te[t]
        assert pos == start + n
        assert toff[i + 1] - toff[i] == -(-n // task_samples)
        start += n
    assert plan.nsamples == start
    return plan


def test_plan_puts_every_sample_in_one_task_of_its_slice():
    check_plan([5, 0, 7, 1], 8)            # an empty slice: no task
    check_plan([0, 0, 100, 0], 1000)       # one slice holds everything
    p = check_plan([10, 3, 29, 0, 12], 4)  # slices in 3 and more tasks
    assert [b - a for a, b in zip(p.toff.tolist()[:-1], p.toff.tolist()[1:])] == [3, 1, 8, 0, 3]
    with pytest.raises(ValueError):
        _hostops.GradPlan([1], "cpu", 0)


def test_plan_cache_identity_and_version():
    autodiff.clear_plans()
    X = torch.tensor([[0, 1], [2, 1], [2, 3], [1, 0]])
    n0 = autodiff.PLAN_BUILDS
    a = autodiff.plan_for(X[:, 0], 4)
    assert autodiff.PLAN_BUILDS == n0 + 1
    assert autodiff.plan_for(X[:, 0], 4) is a and autodiff.PLAN_BUILDS == n0 + 1  # a fresh view of the same, unmodified base
    autodiff.plan_for(X[:, 1], 4)                                              # another offset
    assert autodiff.PLAN_BUILDS == n0 + 2
    X[0, 0] = 3                                                                 # an in-place write bumps the version
    b = autodiff.plan_for(X[:, 0], 4)
    assert autodiff.PLAN_BUILDS == n0 + 3 and b is not a
    assert b[0].tolist() == [3, 1, 2, 0] and a[0].tolist() == [0, 3, 1, 2]       # stable sorts of [3, 2, 2, 1] and [0, 2, 2, 1]
    autodiff.plan_for(X.clone()[:, 0], 4)                                       # equal values, another tensor object
    assert autodiff.PLAN_BUILDS == n0 + 4
    for _ in range(autodiff.PLAN_CACHE_SIZE + 3):
        autodiff.plan_for(torch.zeros(2, dtype=torch.int64), 4)
    assert len(autodiff._plans) == autodiff.PLAN_CACHE_SIZE
    autodiff.clear_plans()

"""The differentiable point evaluation ``t[X]`` on the device, the losses built on it and ``tn.optimize`` end to end.

Gradients are compared with CPU fp64 autograd of the host mirror on the same dtype-rounded parameters.  Tolerance per element:
2 k eps G_abs, where G_abs is the same gradient computed in fp64 from |cores|, |factors| and |upstream gradient| (the sum of the
absolute values of all monomials) and k = P + sum_n (r_n + 1), plus the Tucker ranks where there are factors, bounds the roundings
along any monomial.  eps = 2^-23 / 2^-52.  Nothing here is measured."""
import pytest
import torch

import tntorch_amd as tn
from tntorch_amd import autodiff

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.float64]
EPS = {torch.float64: 2.0 ** -52, torch.float32: 2.0 ** -23}
F64 = torch.float64


@pytest.fixture(autouse=True)
def small_tasks():
    """Seven samples per task: the slices of these small cases run as one, two and more tasks."""
    old = autodiff.TASK_SAMPLES
    autodiff.TASK_SAMPLES = 7
    autodiff.clear_plans()
    yield
    autodiff.TASK_SAMPLES = old
    autodiff.clear_plans()


def params(ranks, sizes, dtype, seed, tucker=None):
    """CPU fp64 copies of dtype-rounded cores [r_n, S_n, r_{n+1}] and factors [I_n, S_n] (None without a Tucker rank)."""
    g = torch.Generator().manual_seed(seed)
    tucker = tucker or [None] * len(sizes)
    cores, Us = [], []
    for n, I in enumerate(sizes):
        S = I if tucker[n] is None else tucker[n]
        cores.append(torch.randn(ranks[n], S, ranks[n + 1], generator=g, dtype=F64).to(dtype).double())
        Us.append(None if tucker[n] is None else torch.randn(I, S, generator=g, dtype=F64).to(dtype).double())
    return cores, Us


def points(sizes, P, seed, k=None):
    g = torch.Generator().manual_seed(seed)
    k = len(sizes) if k is None else k
    X = torch.stack([torch.randint(-I, I, (P,), generator=g) for I in sizes[:k]], dim=1)  # negative entries wrap
    X[1] = X[0]  # a repeated point
    X[:P // 2, 0] = X[0, 0]  # one long slice in mode 0
    return X


def train(cores, Us, dtype, device, frozen=()):
    def leaf(x, n):
        return None if x is None else x.detach().clone().to(dtype).to(device).requires_grad_(n not in frozen)

    return tn.Tensor([leaf(c, n) for n, c in enumerate(cores)], Us=[leaf(U, n) for n, U in enumerate(Us)])


def grads_of(t, X, W):
    """Gradients of sum(W * t[X].torch()) for every core and factor (None where there is none)."""
    out = t[X].torch()
    (out * W.to(out.dtype).to(out.device)).sum().backward()
    nodes = list(t.cores) + list(t.Us)
    return out.detach(), [None if x is None or x.grad is None else x.grad.detach().cpu().double() for x in nodes]


def check_case(ranks, sizes, dtype, seed, tucker=None, k=None, P=41):
    cores, Us = params(ranks, sizes, dtype, seed, tucker)
    X = points(sizes, P, seed + 1, k)
    shape_out = [P] + list(sizes[X.shape[1]:])
    W = torch.randn(shape_out, generator=torch.Generator().manual_seed(seed + 2), dtype=F64).to(dtype).double()
    out_d, got = grads_of(train(cores, Us, dtype, DEV), X.to(DEV), W)
    out_r, ref = grads_of(train(cores, Us, F64, "cpu"), X, W)
    out_a, mag = grads_of(train([c.abs() for c in cores], [None if U is None else U.abs() for U in Us], F64, "cpu"), X, W.abs())
    kk = P + sum(r + 1 for r in ranks) + sum(s for s in (tucker or []) if s is not None)
    tol = 2 * kk * EPS[dtype]
    assert tuple(out_d.shape) == tuple(shape_out)
    assert bool(((out_d.cpu().double() - out_r).abs() <= tol * out_a).all())
    for a, b, m in zip(got, ref, mag):
        assert (a is None) == (b is None)
        if a is not None:
            err = (a - b).abs()
            assert bool((err <= tol * m).all()), float((err / (tol * m).clamp_min(1e-300)).max())
    return got


@pytest.mark.parametrize("dtype", DTYPES)
def test_gradients_tt_all_modes_indexed(dtype):
    check_case([1, 3, 17, 1], [4, 5, 6], dtype, 10)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gradients_tt_tucker(dtype):
    check_case([1, 3, 4, 1], [6, 5, 7], dtype, 20, tucker=[3, None, 4])


@pytest.mark.parametrize("dtype", DTYPES)
def test_gradients_with_a_trailing_mode(dtype):
    check_case([1, 4, 5, 1], [5, 4, 3], dtype, 30, k=2)
    check_case([1, 4, 5, 1], [5, 4, 3], dtype, 31, tucker=[None, None, 2], k=2)  # the trailing mode keeps its factor


def test_frozen_middle_core():
    dtype = torch.float32
    cores, Us = params([1, 3, 17, 1], [4, 5, 6], dtype, 40)
    X = points([4, 5, 6], 41, 41).to(DEV)
    W = torch.randn(41, generator=torch.Generator().manual_seed(42), dtype=F64)
    _, full = grads_of(train(cores, Us, dtype, DEV), X, W)
    t = train(cores, Us, dtype, DEV, frozen=(1,))
    _, part = grads_of(t, X, W)
    assert t.cores[1].grad is None and part[1] is None
    assert torch.equal(part[0], full[0]) and torch.equal(part[2], full[2])


def test_gradcheck_of_the_function():
    cores, _ = params([1, 2, 2, 1], [3, 3, 3], F64, 50)
    X = torch.tensor([[0, 1, 2], [2, 2, 0], [0, 1, 2], [1, -1, 1], [-3, 0, -2]], device=DEV)
    leaves = [c.to(DEV).requires_grad_() for c in cores]
    cols = [X[:, n] for n in range(3)]
    assert torch.autograd.gradcheck(lambda *c: autodiff.point_eval(c, cols), leaves)
    assert torch.autograd.gradcheck(lambda *c: autodiff.point_eval(c, cols[:2]), leaves[:2])  # r_b = 2


@pytest.mark.parametrize("dtype", DTYPES)
def test_values_match_the_no_grad_path_and_plans_are_cached(dtype):
    ranks, sizes, P = [1, 3, 17, 1], [4, 5, 6], 41
    cores, Us = params(ranks, sizes, dtype, 60)
    X = points(sizes, P, 61).to(DEV)
    t = train(cores, Us, dtype, DEV)
    plain = tn.Tensor([c.detach() for c in t.cores])[X].torch()  # ttr_gather_chain
    n0 = autodiff.PLAN_BUILDS
    v1 = t[X].torch()
    assert autodiff.PLAN_BUILDS == n0 + 3
    v2 = t[X].torch()
    assert autodiff.PLAN_BUILDS == n0 + 3 and torch.equal(v1, v2)  # the same unmodified X: no plan is built
    mag = tn.Tensor([c.abs() for c in cores])[X.cpu()].torch()
    kk = P + sum(r + 1 for r in ranks)
    assert bool(((v1.detach() - plain).abs().cpu().double() <= 2 * kk * EPS[dtype] * mag).all())
    print("values under grad bitwise equal to ttr_gather_chain:", torch.equal(v1.detach(), plain))
    X[0, 0] = 1  # an in-place change: the plans of X's columns are rebuilt
    t[X].torch()
    assert autodiff.PLAN_BUILDS == n0 + 6


def test_out_of_range_index_and_no_points():
    cores, Us = params([1, 2, 3, 1], [4, 5, 6], torch.float32, 70)
    t = train(cores, Us, torch.float32, DEV)
    X = points([4, 5, 6], 9, 71)
    X[3, 1] = 5
    with pytest.raises(IndexError, match="index out of range"):
        t[X.to(DEV)]
    assert all(c.grad is None for c in t.cores)
    out = t[torch.zeros((0, 3), dtype=torch.int64, device=DEV)].torch()
    assert tuple(out.shape) == (0,)
    out.sum().backward()
    for c in t.cores:
        assert c.grad is not None and c.grad.shape == c.shape and not c.grad.any()


def test_loss_gradients_against_torch_on_the_cpu():
    """fp64 on both sides; the two differ by roundings of relative size ~k eps ~ 1e-14 of well-conditioned sums (the distance is
    far from zero), so 1e-10 of the largest gradient entry leaves four digits for cancellation."""
    cores, Us = params([1, 3, 4, 1], [4, 5, 6], F64, 80, tucker=[None, 3, None])
    X = points([4, 5, 6], 30, 81)
    y = torch.randn(30, generator=torch.Generator().manual_seed(82), dtype=F64)
    for loss in (lambda y, t, X: tn.relative_error(y, t[X]), lambda y, t, X: tn.dist(t[X], y), lambda y, t, X: tn.dist(y, t[X].torch())):
        td, tc = train(cores, Us, F64, DEV), train(cores, Us, F64, "cpu")
        ld, lc = loss(y.to(DEV), td, X.to(DEV)), loss(y, tc, X)
        assert abs(float(ld.detach()) - float(lc.detach())) <= 1e-12 * abs(float(lc.detach()))
        ld.backward()
        lc.backward()
        for a, b in zip(list(td.cores) + [td.Us[1]], list(tc.cores) + [tc.Us[1]]):
            assert float((a.grad.cpu() - b.grad).abs().max()) <= 1e-10 * float(b.grad.abs().max())
    a = torch.randn(7, dtype=F64, device=DEV).requires_grad_()  # dist == 0: zero gradients, not NaN
    tn.dist(a, a.detach().clone()).backward()
    assert not a.grad.any() and not a.grad.isnan().any()


def test_refusals_survive():
    cores, Us = params([1, 2, 3, 1], [4, 5, 6], torch.float32, 90)
    t = train(cores, Us, torch.float32, DEV)
    idx = torch.tensor([0, 1, 2], device=DEV)
    with pytest.raises(NotImplementedError):
        t.clone().round_tt(rmax=2)
    with pytest.raises(NotImplementedError):
        tn.dot(t, t)
    with pytest.raises(NotImplementedError):
        tn.partialset(t)
    with pytest.raises(NotImplementedError):
        t[:, idx]            # the index block does not start at mode 0
    with pytest.raises(NotImplementedError):
        t[0, idx, idx]
    with pytest.raises(NotImplementedError):
        tn.dot(t[idx, idx, idx].torch(), torch.ones(3, device=DEV))  # a dense operand that requires grad
    b = tn.Tensor([torch.randn(2, 1, 3, 2, device=DEV, requires_grad=True), torch.randn(2, 2, 3, 1, device=DEV, requires_grad=True)],
                  batch=True)
    with pytest.raises(NotImplementedError):
        b[:, idx, idx]
    cp = tn.Tensor([torch.randn(4, 2, device=DEV, requires_grad=True), torch.randn(5, 2, device=DEV, requires_grad=True)])
    with pytest.raises(NotImplementedError):
        cp[idx, idx]
    with torch.no_grad():  # grad mode off: today's refusal, untouched
        with pytest.raises(NotImplementedError):
            t[idx, idx, idx]


@pytest.mark.parametrize("dtype", DTYPES)
def test_optimize_on_the_device(dtype):
    cores, Us = params([1, 2, 2, 1], [4, 4, 4], dtype, 100)
    X = torch.cartesian_prod(*[torch.arange(4)] * 3).to(DEV)
    y = tn.Tensor([c.to(dtype).to(DEV) for c in cores])[X].torch()
    start_cores, _ = params([1, 2, 2, 1], [4, 4, 4], dtype, 101)
    t = train(start_cores, Us, dtype, DEV)
    start = float(tn.relative_error(y, t[X]).detach())
    n0 = autodiff.PLAN_BUILDS
    tn.optimize(t, lambda t: tn.relative_error(y, t[X]), max_iter=50, verbose=False)
    assert autodiff.PLAN_BUILDS == n0  # the plans of X's columns were built by the evaluation above, once
    end = float(tn.relative_error(y, t[X]).detach())
    assert end < start
    assert all(c.is_cuda and bool(torch.isfinite(c).all()) and c.grad is not None and bool(c.grad.any()) for c in t.cores)
    assert tn.dof(t) == 8 + 16 + 8

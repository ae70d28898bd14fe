"""The differentiable ``tn.tt_multiply`` on a real MI355X through the public API: gradcheck, the gradients of every core and of the
tensor against CPU fp64 autograd within the derived chain bounds of matrix_grad_cases, the forward's bits, which launches a
backward pass costs, a short Adam fit against the same fit on the CPU, and that ``cp_multiply`` refuses instead of cutting the graph."""
import numpy as np
import pytest
import torch

import matrix_cases as mc
import matrix_grad_cases as gc
import tntorch_amd as tn
from tntorch_amd import _hip

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]


def _dims(name):
    return mc.RANDOM_CASES[gc.GRAD_CASES[name][0]][:2]


def _leaves(name, dt, frozen=(), x_grad=True):
    tt, x, w = gc.operands(name, dt)
    cores = [c.cuda().requires_grad_(k not in frozen) for k, c in enumerate(tt)]
    return cores, x.cuda().requires_grad_(x_grad), w.cuda()


def _count(monkeypatch):
    calls = []
    real = _hip._call

    def counting(name, *args):
        calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(_hip, "_call", counting)
    return calls


def test_gradcheck():
    g = torch.Generator().manual_seed(4)
    G0 = torch.randn((1, 2, 3, 2), dtype=torch.float64, generator=g).cuda().requires_grad_()
    G1 = torch.randn((2, 3, 2, 1), dtype=torch.float64, generator=g).cuda().requires_grad_()
    x = torch.randn((3, 6), dtype=torch.float64, generator=g).cuda().requires_grad_()
    assert torch.autograd.gradcheck(lambda x, a, b: tn.tt_multiply(tn.TTMatrix([a, b], None, [2, 3], [3, 2]), x), (x, G0, G1))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(gc.GRAD_CASES))
def test_gradients_against_cpu_fp64_autograd(name, dt):
    idims, odims = _dims(name)
    cores, x, w = _leaves(name, dt)
    y64, dG64, dx64, bG, bx = gc.truth_and_bounds(name, dt)
    y = tn.tt_multiply(tn.TTMatrix(cores, None, idims, odims), x)
    assert y.is_cuda and y.dtype == dt and y.grad_fn is not None
    with torch.no_grad():
        plain = tn.tt_multiply(tn.TTMatrix([c.detach() for c in cores], None, idims, odims), x.detach())
    assert plain.grad_fn is None and torch.equal(y.detach(), plain)       # the forward under grad: bitwise the one without
    _, fbound = mc.tt_truth_and_bound([c.detach().cpu() for c in cores], x.detach().cpu(), dt)
    mc.assert_within(y, y64, fbound, "{} {} y".format(name, dt))
    (y * w).sum().backward()
    for k, c in enumerate(cores):
        assert c.grad.is_cuda and c.grad.dtype == dt and c.grad.shape == c.shape
        mc.assert_within(c.grad, dG64[k], bG[k], "{} {} dG{}".format(name, dt, k))
    assert x.grad.is_cuda and x.grad.dtype == dt and x.grad.shape == x.shape
    mc.assert_within(x.grad, dx64, bx, "{} {} dx".format(name, dt))
    first = [c.grad.clone() for c in cores] + [x.grad.clone()]
    for t in cores + [x]:
        t.grad = None
    (tn.tt_multiply(tn.TTMatrix(cores, None, idims, odims), x) * w).sum().backward()
    assert all(torch.equal(a, b.grad) for a, b in zip(first, cores + [x]))   # the same bits every time


@pytest.mark.parametrize("dt", DTYPES)
def test_tensor_with_more_dimensions(dt):
    """The tensor is reshaped by torch on the way in, so its gradient comes back in its own shape."""
    idims, odims = _dims("three")
    cores, x, w = _leaves("three", dt)
    x3 = x.detach().reshape(3, 3, 60).clone().requires_grad_()
    (tn.tt_multiply(tn.TTMatrix(cores, None, idims, odims), x3) * w).sum().backward()
    _, _, dx64, _, bx = gc.truth_and_bounds("three", dt)
    assert x3.grad.shape == x3.shape
    mc.assert_within(x3.grad.reshape(9, 60), dx64, bx, "three {} dx of a 3-D tensor".format(dt))


def test_launch_counts(monkeypatch):
    idims, odims = _dims("three")
    d = 3
    calls = _count(monkeypatch)

    def run(frozen=(), x_grad=True):
        cores, x, w = _leaves("three", torch.float32, frozen, x_grad)
        del calls[:]
        (tn.tt_multiply(tn.TTMatrix(cores, None, idims, odims), x) * w).sum().backward()
        return cores, x, {n: calls.count(n) for n in set(calls)}

    cores, x, seen = run()
    assert seen == {"ttr_ttm_step": d, "ttr_ttm_grad_core": d, "ttr_ttm_grad_input": d}       # and no ttr_gemm
    cores, x, seen = run(x_grad=False)
    assert seen == {"ttr_ttm_step": d, "ttr_ttm_grad_core": d, "ttr_ttm_grad_input": d - 1} and x.grad is None
    cores, x, seen = run(frozen=(0, 1), x_grad=False)
    assert seen == {"ttr_ttm_step": d, "ttr_ttm_grad_core": 1} and cores[2].grad is not None
    assert cores[0].grad is None and cores[1].grad is None and x.grad is None
    cores, x, seen = run(frozen=(1,))
    assert seen == {"ttr_ttm_step": d, "ttr_ttm_grad_core": d - 1, "ttr_ttm_grad_input": d}
    assert cores[1].grad is None and cores[0].grad is not None and cores[2].grad is not None   # a frozen core gets no .grad
    cores, x, _ = _leaves("three", torch.float32)
    del calls[:]
    with torch.no_grad():
        y = tn.tt_multiply(tn.TTMatrix(cores, None, idims, odims), x.detach())
    assert calls == ["ttr_ttm_step"] * d and y.grad_fn is None                              # today's path, untouched


@pytest.mark.parametrize("dt", DTYPES)
def test_short_fit(dt):
    """Adam on device cores against y = x @ M_true, and the same fit from the same start on the CPU mirror in fp64.  60 steps at
    lr = 0.05 were chosen on the CPU, where they lower the loss about 28-fold: the CPU run must reach 10-fold, the device 5-fold."""
    idims, odims, ranks, b, steps = [4, 3, 2], [2, 3, 4], [3, 3], 48, 60
    g = torch.Generator().manual_seed(21)
    rk = [1] + ranks + [1]

    def draw():
        return [0.5 * torch.randn((rk[k], idims[k], odims[k], rk[k + 1]), dtype=torch.float64, generator=g) for k in range(3)]

    true, start = draw(), draw()
    x = torch.randn((b, int(np.prod(idims))), dtype=torch.float64, generator=g)
    y = x @ mc.tt_dense(true)

    def fit(cores, x, y):
        opt = torch.optim.Adam(cores, lr=0.05)
        ttm = tn.TTMatrix(cores, None, idims, odims)
        losses = []
        for _ in range(steps + 1):
            opt.zero_grad()
            loss = ((tn.tt_multiply(ttm, x) - y) ** 2).mean()
            loss.backward()
            opt.step()
            losses.append(loss.detach())
        return float(losses[0]), float(losses[-1])

    first, last = fit([c.clone().requires_grad_() for c in start], x, y)
    print("cpu fp64: loss {:.4e} -> {:.4e} ({:.1f}x)".format(first, last, first / last))
    assert first >= 10 * last
    dfirst, dlast = fit([c.to(dt).cuda().requires_grad_() for c in start], x.to(dt).cuda(), y.to(dt).cuda())
    print("device {}: loss {:.4e} -> {:.4e} ({:.1f}x)".format(dt, dfirst, dlast, dfirst / dlast))
    assert dfirst >= 5 * dlast


def test_cp_multiply_refuses_instead_of_cutting_the_graph():
    idims, odims = mc.RANDOM_CASES["three"][:2]
    _, cp, x = mc.random_cores("three", torch.float64)
    cores = [c.cuda().requires_grad_() for c in cp]
    cpm = tn.CPMatrix(cores, None, idims, odims)
    with pytest.raises(NotImplementedError):
        tn.cp_multiply(cpm, x.cuda())
    with pytest.raises(NotImplementedError):
        tn.cp_multiply(tn.CPMatrix([cores[0]] + [c.detach() for c in cores[1:]], None, idims, odims), x.cuda())
    with pytest.raises(NotImplementedError):
        tn.cp_multiply(tn.CPMatrix([c.detach() for c in cores], None, idims, odims), x.cuda().requires_grad_())
    with torch.no_grad():
        z = tn.cp_multiply(cpm, x.cuda())
    z64, zbound = mc.cp_truth_and_bound(cp, x, torch.float64)
    mc.assert_within(z, z64, zbound, "cp_multiply under no_grad")
    assert z.grad_fn is None

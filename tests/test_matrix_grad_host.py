"""The differentiable ``tn.tt_multiply`` without a GPU: the bookkeeping of ``autodiff.tt_matvec`` run with the host mirror as its
``ops`` against plain torch autograd of the einsum chain (fp64, 1e-12 relative), which operands cost a call and which do not, the
three host mirrors against their definitions, the declarations of the new entries, and that the CPU products stay plain torch."""
import os
import re

import pytest
import torch

import matrix_cases as mc
import matrix_grad_cases as gc
import tntorch_amd as tn
from tntorch_amd import _hip, _hostops, autodiff

NEW_ENTRIES = ("ttr_ttm_grad_input", "ttr_ttm_grad_core_slab_rows", "ttr_ttm_grad_core_workspace_bytes", "ttr_ttm_grad_core")


class CountingOps:
    """The host mirror's three step functions, recording every call: (name, shape of what it returned)."""

    def __init__(self):
        self.calls = []

    def _wrap(self, name, *args):
        out = getattr(_hostops, name)(*args)
        self.calls.append((name, tuple(out.shape)))
        return out

    def ttm_step(self, X, G):
        return self._wrap("ttm_step", X, G)

    def ttm_grad_input(self, dY, G):
        return self._wrap("ttm_grad_input", dY, G)

    def ttm_grad_core(self, X, dY):
        return self._wrap("ttm_grad_core", X, dY)

    def count(self, name):
        return sum(1 for n, _ in self.calls if n == name)


def _close(a, b, what):
    err = float((a - b).abs().max())
    scale = float(b.abs().max())
    print("{}: largest difference {:.3e} at scale {:.3e}".format(what, err, scale))
    assert a.shape == b.shape and err <= 1e-12 * scale, what


def _run(name, frozen=(), x_grad=True):
    """The Function over CountingOps for a case in fp64; (ops, y, cores, x, expected y, expected core grads, expected dx)."""
    tt, x, w = gc.operands(name, torch.float64)
    ey, eG, ex = gc.autograd_grads(tt, x, w)
    cores = [c.clone().requires_grad_(k not in frozen) for k, c in enumerate(tt)]
    xx = x.clone().requires_grad_(x_grad)
    ops = CountingOps()
    y = autodiff.tt_matvec(cores, xx, ops)
    (y * w).sum().backward()
    return ops, y, cores, xx, ey, eG, ex


@pytest.mark.parametrize("name", list(gc.GRAD_CASES))
def test_function_over_the_host_mirror_matches_autograd(name):
    ops, y, cores, x, ey, eG, ex = _run(name)
    d = len(cores)
    assert torch.equal(y.detach(), _hostops.tt_matvec_chain([c.detach() for c in cores], x.detach()))
    _close(y.detach(), ey, "{} y".format(name))
    for k in range(d):
        _close(cores[k].grad, eG[k], "{} dG{}".format(name, k))
    _close(x.grad, ex, "{} dx".format(name))
    assert x.grad.is_contiguous() and all(c.grad.is_contiguous() for c in cores)
    assert (ops.count("ttm_step"), ops.count("ttm_grad_core"), ops.count("ttm_grad_input")) == (d, d, d)


@pytest.mark.parametrize("name", ["ref", "three", "b1"])
def test_one_core_frozen(name):
    d = len(gc.operands(name, torch.float64)[0])
    for frozen in range(d):
        ops, y, cores, x, ey, eG, ex = _run(name, frozen=(frozen,))
        assert cores[frozen].grad is None
        for k in range(d):
            if k != frozen:
                _close(cores[k].grad, eG[k], "{} frozen {} dG{}".format(name, frozen, k))
        _close(x.grad, ex, "{} frozen {} dx".format(name, frozen))
        assert ops.count("ttm_grad_core") == d - 1 and ops.count("ttm_grad_input") == d
        assert tuple(cores[frozen].shape) not in [s for n, s in ops.calls if n == "ttm_grad_core"]   # no grad_core for the frozen core


@pytest.mark.parametrize("name", list(gc.GRAD_CASES))
def test_x_without_grad_costs_no_step_0(name):
    ops, y, cores, x, ey, eG, ex = _run(name, x_grad=False)
    d = len(cores)
    assert x.grad is None
    for k in range(d):
        _close(cores[k].grad, eG[k], "{} dG{}".format(name, k))
    assert ops.count("ttm_grad_core") == d and ops.count("ttm_grad_input") == d - 1
    I0, D0 = cores[0].shape[1], x.numel() // cores[0].shape[1]
    assert (I0, D0, 1) not in [s for n, s in ops.calls if n == "ttm_grad_input"]   # no grad_input at step 0


def test_only_the_last_core_and_only_x():
    ops, y, cores, x, ey, eG, ex = _run("three", frozen=(0, 1), x_grad=False)
    assert ops.count("ttm_grad_core") == 1 and ops.count("ttm_grad_input") == 0
    _close(cores[2].grad, eG[2], "last core")
    assert cores[0].grad is None and cores[1].grad is None and x.grad is None
    ops, y, cores, x, ey, eG, ex = _run("three", frozen=(0, 1, 2), x_grad=True)
    assert ops.count("ttm_grad_core") == 0 and ops.count("ttm_grad_input") == 3
    _close(x.grad, ex, "only x")
    assert all(c.grad is None for c in cores)


def test_host_mirrors_are_their_definitions_exactly():
    """Asymmetric small integers: every product and sum is exact, so a mirror must EQUAL its definition written out as loops over
    the summed indices -- a transposed index pair would show whatever the tolerance."""
    I, D, R, O, S = 3, 5, 4, 2, 6
    dt = torch.float64
    X = gc.small_integers((I, D, R), 7, 11, dt)
    G = gc.small_integers((R, I, O, S), 5, 13, dt)
    dY = gc.small_integers((D, O, S), 3, 7, dt)
    Y = torch.zeros((D, O, S), dtype=dt)
    dX = torch.zeros((I, D, R), dtype=dt)
    dG = torch.zeros((R, I, O, S), dtype=dt)
    for i in range(I):
        for r in range(R):
            Y += X[i, :, r][:, None, None] * G[r, i][None]                 # Y[dd, o, s] += X[i, dd, r] G[r, i, o, s]
            dX[i, :, r] = (dY * G[r, i][None]).sum(dim=(1, 2))             # dX[i, dd, r] = sum_{o, s} dY[dd, o, s] G[r, i, o, s]
            dG[r, i] = (X[i, :, r][:, None, None] * dY).sum(dim=0)         # dG[r, i, o, s] = sum_dd X[i, dd, r] dY[dd, o, s]
    for got, want in ((_hostops.ttm_step(X, G), Y), (_hostops.ttm_grad_input(dY, G), dX), (_hostops.ttm_grad_core(X, dY), dG)):
        assert got.shape == want.shape and got.is_contiguous() and torch.equal(got, want)


def test_declarations():
    root = mc.ROOT
    with open(os.path.join(root, "include", "ttround_hip.h")) as f:
        header = f.read()
    define = header.index("#define TTR_ABI_VERSION")
    for name in NEW_ENTRIES:
        assert name in header[:define], "{} is not named in the comment above TTR_ABI_VERSION".format(name)
        assert re.search(r"\bint(64_t)?\s+{}\s*\(".format(name), header[define:]), name
        assert name in _hip.EXPORTED_SYMBOLS
    assert _hip.ABI_VERSION == 17
    with open(os.path.join(root, "tntorch_amd", "csrc", "Makefile")) as f:
        assert "ttr_ttmatrix_grad.hip" in f.read().replace("\\\n", " ").split()
    assert tn.matrix.__all__ == ["TTMatrix", "CPMatrix", "tt_multiply", "cp_multiply"]
    assert tn.autodiff.__all__ == ["optimize", "dof"]
    for name in ("ttm_grad_input", "ttm_grad_core", "ttm_grad_core_slab_rows", "ttm_grad_core_workspace_bytes"):
        assert callable(getattr(_hip, name))


@pytest.mark.parametrize("name", ["ref", "three"])
def test_cpu_products_still_differentiate_through_torch(name):
    idims, odims = mc.RANDOM_CASES[name][:2]
    tt, cp, x = mc.random_cores(name, torch.float64)
    for kind, mul, raw, dense in ((tn.TTMatrix, tn.tt_multiply, tt, mc.tt_dense), (tn.CPMatrix, tn.cp_multiply, cp, mc.cp_dense)):
        cores = [c.clone().requires_grad_(True) for c in raw]
        xx = x.clone().requires_grad_(True)
        y = mul(kind(cores, None, idims, odims), xx)
        assert y.grad_fn is not None
        y.sum().backward()
        assert all(c.grad is not None and bool(c.grad.abs().sum() > 0) for c in cores)
        want = dense(raw).sum(dim=1)[None, :].expand_as(x)                 # d(sum(x M)) / dx = the row sums of M
        assert torch.allclose(xx.grad, want, rtol=1e-10, atol=1e-10)

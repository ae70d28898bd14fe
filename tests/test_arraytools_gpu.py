"""The array tools (``tn.cat``, ``tn.flip``, ``tn.ttm``, ``tn.cumsum``, ``tn.pad``, ...) on device trains on a real MI355X: every
case of tests/golden/arraytools_f64.npz and every dense truth of the host file, to the same tolerances (relative Frobenius 1e-12
in fp64, 1e-5 in fp32), with the results on the device in the input's dtype; the matrix ``ttm`` against the fp64 product within
the dot-product bound 2 I u (|U| |X|) per entry, u = 2^-24 / 2^-53; and ``cumsum`` / the vector ``ttm`` on the long edge cores
1 x 4096 x 64 and 64 x 4096 x 1 against the fp64 host mirror within the kernels' derived bounds."""
import pytest
import torch

import arraytools_cases as ac
import tntorch_amd as tn
from tntorch_amd import _hostops

pytestmark = pytest.mark.gpu

DTYPES = [torch.float64, torch.float32]


def _on_device(out, dt):
    for x in (out if isinstance(out, list) else [out]):
        tensors = (list(x.cores) + [U for U in x.Us if U is not None]) if hasattr(x, "cores") else [x]
        assert all(c.is_cuda and c.dtype == dt for c in tensors)


@pytest.fixture(scope="module", params=DTYPES, ids=["f64", "f32"])
def device_inputs(request):
    T, A = ac.inputs(request.param, "cuda")
    return request.param, T, A, ac.snapshot(T, A)


@pytest.mark.parametrize("case", ac.cases())
def test_golden(case, device_inputs):
    dt, T, A, snap = device_inputs
    out = ac.CASES[case](tn, T, A)
    _on_device(out, dt)
    err = ac.rel_err(ac.dense(out), ac.truth(case))
    print(case, dt, "relative error", err)
    assert err <= ac.tol(dt)
    assert ac.unchanged(T, A, snap)


@pytest.mark.parametrize("case", sorted(ac.DENSE_TRUTHS))
def test_dense_truth(case, device_inputs):
    dt, T, A, snap = device_inputs
    out, truth = ac.DENSE_TRUTHS[case](tn, T, A)
    _on_device(out, dt)
    err = ac.rel_err(ac.dense(out), truth)
    print(case, dt, "relative error", err)
    assert err <= ac.tol(dt)
    assert ac.unchanged(T, A, snap)


def test_squeeze_of_all_singletons_is_a_device_scalar():
    g = torch.Generator().manual_seed(1)
    t = ac.rand_train([1, 1, 1], 2, g, torch.float64, device="cuda")
    out = tn.squeeze(t)
    assert torch.is_tensor(out) and out.dim() == 0 and out.is_cuda
    assert abs(float(out) - float(ac.dense(t).reshape(()))) < 1e-14


@pytest.mark.parametrize("dt", DTYPES)
def test_reduce_with_cat(dt):
    out, truth = ac.reduce_cat(tn, dt, device="cuda")
    _on_device(out, dt)
    assert ac.rel_err(ac.dense(out), truth) <= ac.tol(dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("transpose", [False, True])
def test_ttm_matrix_within_the_dot_product_bound(dt, transpose):
    """Per entry of the new core: |sum_i U[j, i] X[r, i, c] - fp64| <= 2 I u sum_i |U[j, i]| |X[r, i, c]| for any summation order."""
    g = torch.Generator().manual_seed(3)
    t = ac.rand_train([5, 37, 6], 3, g, dt, tucker=(2,), device="cuda")
    M = torch.randn(19, 37, generator=g, dtype=torch.float64).to(dt)
    U2 = torch.randn(4, 6, generator=g, dtype=torch.float64).to(dt)
    out = tn.ttm(t, [(M.t() if transpose else M).cuda(), (U2.t() if transpose else U2).cuda()], dim=[1, 2], transpose=transpose)
    _on_device(out, dt)
    assert tuple(out.shape) == (5, 19, 4) and out.Us[2] is not None and torch.equal(out.cores[2], t.cores[2])
    u = ac.U32 if dt == torch.float32 else ac.U64
    X = t.cores[1].cpu().double()
    truth = torch.einsum("ji,ric->rjc", M.double(), X)
    bound = 2 * 37 * u * torch.einsum("ji,ric->rjc", M.double().abs(), X.abs())
    assert bool(((out.cores[1].cpu().double() - truth).abs() <= bound).all())
    F = t.Us[2].cpu().double()   # the Tucker mode keeps its structure: factor @ Us[n]
    assert bool(((out.Us[2].cpu().double() - U2.double() @ F).abs() <= 2 * 6 * u * (U2.double().abs() @ F.abs())).all())


@pytest.mark.parametrize("dt", DTYPES)
def test_long_edge_cores_against_the_host_mirror(dt):
    """A 4096 x 4096 train of rank 64: the first core 1 x 4096 x 64 and the last core 64 x 4096 x 1."""
    g = torch.Generator().manual_seed(4)
    cores = [torch.randn(1, 4096, 64, generator=g, dtype=torch.float64).to(dt), torch.randn(64, 4096, 1, generator=g, dtype=torch.float64).to(dt)]
    w = torch.randn(4096, generator=g, dtype=torch.float64).to(dt)
    t = tn.Tensor([c.cuda() for c in cores])
    scanned = tn.cumsum(t)
    reduced = tn.ttm(t, [w.cuda(), w.cuda()])
    _on_device(scanned, dt)
    _on_device(reduced, dt)
    assert tuple(reduced.shape) == (1, 1)
    for n, X in enumerate(cores):
        truth, A = ac.scan_truth(X)
        mirror = _hostops.mode_scan(X)
        assert float((mirror.double() - truth).abs().max()) <= 2.0 ** -23 * float(truth.abs().max())   # the mirror rounds the fp64 scan once
        err = (scanned.cores[n].cpu().double() - truth).abs()
        assert bool((err <= ac.kernel_bound("scan", 4096, dt, truth, A)).all()), (n, float(err.max()))
        truth, A = ac.reduce_truth(X, w, 1.0)
        err = (reduced.cores[n][:, 0, :].cpu().double() - truth).abs()
        assert bool((err <= ac.kernel_bound("reduce", 4096, dt, truth, A)).all()), (n, float(err.max()))
        assert bool(((_hostops.mode_reduce(X, w).double() - truth).abs() <= ac.kernel_bound("reduce", 4096, dt, truth, A)).all())
    assert all(torch.equal(a.cpu(), b) for a, b in zip(t.cores, cores))

"""``tn.tt_multiply`` / ``tn.cp_multiply`` / ``tn.CPMatrix`` on a real MI355X: the cases of tests/test_matrix_host.py on the device,
against the CPU fp64 truth and the outputs the reference recorded, within the derived chain bounds of matrix_cases; that the
result stays on the device in the operands' dtype; the constructors on device tensors; and that the device path is exactly ``d``
launches of ttr_ttm_step (ttr_cpm_step and one ttr_mode_reduce) and no GEMM."""
import pytest
import torch

import matrix_cases as mc
import tntorch_amd as tn
from tntorch_amd import _hip

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]


def _matrices(name, dt):
    idims, odims = mc.RANDOM_CASES[name][:2]
    tt, cp, x = mc.random_cores(name, dt)
    return (tn.TTMatrix([c.cuda() for c in tt], None, idims, odims), tn.CPMatrix([c.cuda() for c in cp], None, idims, odims), x.cuda(),
            tt, cp, x)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(mc.RANDOM_CASES))
def test_products_on_the_device(name, dt):
    ttm, cpm, xd, tt, cp, x = _matrices(name, dt)
    y = tn.tt_multiply(ttm, xd)
    assert y.is_cuda and y.device == xd.device and y.dtype == dt and tuple(y.shape) == (x.shape[0], int(torch.prod(ttm.output_dims)))
    y64, bound = mc.tt_truth_and_bound(tt, x, dt)
    mc.assert_within(y, y64, bound, "tt_multiply {} {}".format(name, dt))
    z = tn.cp_multiply(cpm, xd)
    assert z.is_cuda and z.dtype == dt and tuple(z.shape) == tuple(y.shape)
    z64, zbound = mc.cp_truth_and_bound(cp, x, dt)
    mc.assert_within(z, z64, zbound, "cp_multiply {} {}".format(name, dt))
    assert torch.equal(y, tn.tt_multiply(ttm, xd)) and torch.equal(z, tn.cp_multiply(cpm, xd))   # the same bits every time
    assert torch.equal(xd.cpu(), x) and all(torch.equal(a.cpu(), b) for a, b in zip(ttm.cores + cpm.cores, tt + cp))


@pytest.mark.parametrize("dt", DTYPES)
def test_tensor_with_more_dimensions_and_without_contiguity(dt):
    ttm, cpm, _, tt, cp, _ = _matrices("three", dt)
    rows = 60
    g = torch.Generator().manual_seed(9)
    v3 = torch.randn((2, 3, rows), dtype=torch.float64, generator=g).to(dt)
    vt = torch.randn((rows, 7), dtype=torch.float64, generator=g).to(dt)
    for v in (v3.cuda(), vt.cuda().t()):
        flat = v.cpu().reshape(-1, rows)
        y64, bound = mc.tt_truth_and_bound(tt, flat, dt)
        mc.assert_within(tn.tt_multiply(ttm, v), y64, bound, "tt {}".format(tuple(v.shape)))
        z64, zbound = mc.cp_truth_and_bound(cp, flat, dt)
        mc.assert_within(tn.cp_multiply(cpm, v), z64, zbound, "cp {}".format(tuple(v.shape)))
    cores = [torch.cat([c, c], dim=2)[:, :, :c.shape[2], :] for c in ttm.cores]    # non-contiguous cores: copied, as plumbing
    y64, bound = mc.tt_truth_and_bound(tt, v3.reshape(-1, rows), dt)
    mc.assert_within(tn.tt_multiply(tn.TTMatrix(cores, None, [4, 3, 5], [2, 6, 3]), v3.cuda()), y64, bound, "strided cores")
    for y in (tn.tt_multiply(ttm, torch.zeros((0, rows), dtype=dt).cuda()), tn.cp_multiply(cpm, torch.zeros((0, rows), dtype=dt).cuda())):
        assert y.is_cuda and tuple(y.shape) == (0, 36) and y.dtype == dt


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(mc.CASES))
def test_golden_products_on_the_device(name, dt):
    idims, odims = mc.CASES[name][:2]
    gd = mc.golden(name, dt, "cuda")
    _, bound = mc.tt_truth_and_bound(gd["tt"], gd["x"], dt, doubled=True)
    mc.assert_within(tn.tt_multiply(tn.TTMatrix(gd["tt"], None, idims, odims), gd["x"]), gd["tty"], bound, "golden tt {} {}".format(name, dt))
    _, zbound = mc.cp_truth_and_bound(gd["cp"], gd["x"], dt, doubled=True)
    mc.assert_within(tn.cp_multiply(tn.CPMatrix(gd["cp"], None, idims, odims), gd["x"]), gd["cpy"], zbound, "golden cp {} {}".format(name, dt))


def test_refusals_on_the_device():
    ttm, cpm, xd, _, _, x = _matrices("three", torch.float64)
    for mul, mat in ((tn.tt_multiply, ttm), (tn.cp_multiply, cpm)):
        with pytest.raises(ValueError, match="same device"):
            mul(mat, x)                                   # a CPU tensor with a device matrix
        with pytest.raises(ValueError, match="same dtype"):
            mul(mat, xd.float())
        with pytest.raises(ValueError, match="float32 or float64"):
            mul(mat, xd.half())


def test_ttmatrix_construction_then_product_on_the_device():
    """The reference's `test_tt_multiply` on the device: TT-SVD kernels build the cores, ttr_ttm_step multiplies."""
    torch.manual_seed(1)
    M = torch.rand(33, 46, dtype=torch.float64)
    v = torch.rand(30, 33, dtype=torch.float64)
    ttm = tn.TTMatrix(M.cuda(), [50], [11, 3], [23, 2])
    assert all(c.is_cuda for c in ttm.cores)
    y = tn.tt_multiply(ttm, v.cuda())
    assert y.is_cuda and torch.allclose(y.cpu(), v @ M)


def test_cpmatrix_construction_then_product_on_the_device():
    """The reference's `test_construction` on the device: the CP-ALS kernels build the factors, ttr_cpm_step multiplies."""
    torch.manual_seed(0)
    M = torch.rand(33, 46, dtype=torch.float64)
    v = torch.rand(30, 33, dtype=torch.float64)
    cpm = tn.CPMatrix(M.cuda(), 50, [11, 3], [23, 2])
    assert all(c.is_cuda for c in cpm.cores) and [tuple(c.shape) for c in cpm.cores] == [(11, 23, 50), (3, 2, 50)]
    assert torch.allclose(cpm.torch().cpu(), M)
    y = tn.cp_multiply(cpm, v.cuda())
    assert y.is_cuda and torch.allclose(y.cpu(), v @ cpm.torch().cpu())
    moved = tn.CPMatrix([c.cpu() for c in cpm.cores], None, [11, 3], [23, 2]).to("cuda")
    assert all(c.is_cuda for c in moved.cores) and moved.numpy().shape == (33, 46)


def test_launch_counts(monkeypatch):
    """The device path is d launches of ttr_ttm_step and nothing else from the library; cp: d of ttr_cpm_step + one ttr_mode_reduce."""
    ttm, cpm, xd, _, _, _ = _matrices("three", torch.float32)
    calls = []
    real = _hip._call

    def counting(name, *args):
        calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(_hip, "_call", counting)
    tn.tt_multiply(ttm, xd)
    assert calls == ["ttr_ttm_step"] * 3
    del calls[:]
    tn.cp_multiply(cpm, xd)
    assert calls == ["ttr_cpm_step"] * 3 + ["ttr_mode_reduce"]

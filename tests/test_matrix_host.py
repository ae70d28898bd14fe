"""``tn.tt_multiply``, ``tn.cp_multiply`` and ``tn.CPMatrix`` on the CPU (the host mirror of the device chain): against ``v @ M`` in
fp64 within the derived chain bound of matrix_cases, against the outputs the unmodified reference recorded
(tests/golden/matrix_f64.npz), the refusals, and that the new names are wired through every layer."""
import os
import re

import pytest
import torch

import matrix_cases as mc
import tntorch_amd as tn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float32, torch.float64]


def _matrices(name, dt):
    idims, odims = mc.RANDOM_CASES[name][:2]
    tt, cp, x = mc.random_cores(name, dt)
    return tn.TTMatrix(tt, None, idims, odims), tn.CPMatrix(cp, None, idims, odims), x


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(mc.RANDOM_CASES))
def test_products_equal_v_times_the_dense_matrix(name, dt):
    ttm, cpm, x = _matrices(name, dt)
    keep = [c.clone() for c in ttm.cores + cpm.cores] + [x.clone()]
    y = tn.tt_multiply(ttm, x)
    assert y.dtype == dt and tuple(y.shape) == (x.shape[0], int(torch.prod(ttm.output_dims)))
    y64, bound = mc.tt_truth_and_bound(ttm.cores, x, dt)
    mc.assert_within(y, y64, bound, "tt_multiply {} {}".format(name, dt))
    # the package's own dense matrix says the same (a looser statement: torch() rounds too)
    assert torch.allclose(y.double(), x.double() @ ttm.torch().double(), rtol=0, atol=float(2 * bound.max()))
    z = tn.cp_multiply(cpm, x)
    assert z.dtype == dt and tuple(z.shape) == tuple(y.shape)
    z64, zbound = mc.cp_truth_and_bound(cpm.cores, x, dt)
    mc.assert_within(z, z64, zbound, "cp_multiply {} {}".format(name, dt))
    assert torch.allclose(z.double(), x.double() @ cpm.torch().double(), rtol=0, atol=float(2 * zbound.max()))
    assert all(torch.equal(a, b) for a, b in zip(keep, ttm.cores + cpm.cores + [x]))   # inputs are never modified


@pytest.mark.parametrize("dt", DTYPES)
def test_tensor_with_more_dimensions_and_without_contiguity(dt):
    ttm, cpm, _ = _matrices("three", dt)
    rows = 60
    g = torch.Generator().manual_seed(9)
    v3 = torch.randn((2, 3, rows), dtype=torch.float64, generator=g).to(dt)              # 3-D: b = 6
    v4 = torch.randn((2, 4, 3, 5), dtype=torch.float64, generator=g).to(dt)              # the modes spelled out: b = 2
    wide = torch.randn((rows, 7), dtype=torch.float64, generator=g).to(dt)
    vt = wide.t()                                                                        # non-contiguous [7, rows]
    vs = torch.randn((5, 2 * rows), dtype=torch.float64, generator=g).to(dt)[:, ::2]     # strided columns
    for v in (v3, v4, vt, vs):
        assert v is v3 or v is v4 or not v.is_contiguous()
        flat = v.reshape(-1, rows)
        y64, bound = mc.tt_truth_and_bound(ttm.cores, flat, dt)
        mc.assert_within(tn.tt_multiply(ttm, v), y64, bound, "tt {}".format(tuple(v.shape)))
        z64, zbound = mc.cp_truth_and_bound(cpm.cores, flat, dt)
        mc.assert_within(tn.cp_multiply(cpm, v), z64, zbound, "cp {}".format(tuple(v.shape)))
    # non-contiguous cores (views of wider tensors)
    cores = [torch.cat([c, c], dim=2)[:, :, :c.shape[2], :] for c in ttm.cores]
    assert not all(c.is_contiguous() for c in cores)
    y64, bound = mc.tt_truth_and_bound(ttm.cores, v3.reshape(-1, rows), dt)
    mc.assert_within(tn.tt_multiply(tn.TTMatrix(cores, None, [4, 3, 5], [2, 6, 3]), v3), y64, bound, "strided cores")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(mc.CASES))
def test_golden_products(name, dt):
    """From the cores the reference built, the products match the outputs the reference recorded (bound doubled: the
    reference's own rounding)."""
    idims, odims = mc.CASES[name][:2]
    gd = mc.golden(name, dt)
    ttm = tn.TTMatrix(gd["tt"], None, idims, odims)
    cpm = tn.CPMatrix(gd["cp"], None, idims, odims)
    # fp32: casting the d cores and x perturbs the truth by at most (d + 1) u (|x| . |G| ...), which the second half of the
    # doubled bound covers as it covers the reference's own rounding in fp64
    _, bound = mc.tt_truth_and_bound(gd["tt"], gd["x"], dt, doubled=True)
    mc.assert_within(tn.tt_multiply(ttm, gd["x"]), gd["tty"], bound, "golden tt {} {}".format(name, dt))
    _, zbound = mc.cp_truth_and_bound(gd["cp"], gd["x"], dt, doubled=True)
    mc.assert_within(tn.cp_multiply(cpm, gd["x"]), gd["cpy"], zbound, "golden cp {} {}".format(name, dt))


def test_golden_fixture_is_what_the_tool_draws():
    for name in mc.CASES:
        M, x = mc.draw_matrix(name)
        gd = mc.golden(name)
        assert torch.equal(M, gd["M"]) and torch.equal(x, gd["x"])
        idims, odims, ranks = mc.CASES[name][:3]
        # the reference's TT cores reproduce the matrix where the ranks allow it (case "ref": full rank 6 <= 50)
        if name == "ref":
            assert torch.allclose(tn.TTMatrix(gd["tt"], None, idims, odims).torch(), M)
            assert torch.allclose(gd["tty"], x @ M)


def test_cpmatrix_construction():
    """tests/test_matrix.py:21-22 of the reference: rank 50 on [11, 3] -> [23, 2] reproduces M."""
    torch.manual_seed(0)
    M = torch.rand(33, 46, dtype=torch.float64)
    cpm = tn.CPMatrix(M, 50, [11, 3], [23, 2])
    assert cpm.rank == 50 and cpm.d == 2 and cpm.batch_size == 1
    assert cpm.input_dims.tolist() == [11, 3] and cpm.output_dims.tolist() == [23, 2]
    assert [tuple(c.shape) for c in cpm.cores] == [(11, 23, 50), (3, 2, 50)]
    assert torch.allclose(cpm.torch(), M)
    assert cpm.numpy().shape == (33, 46)
    v = torch.rand(30, 33, dtype=torch.float64)
    assert torch.allclose(tn.cp_multiply(cpm, v), v @ M)
    again = tn.CPMatrix(cpm.cores, None, [11, 3], [23, 2])          # from pre-processed cores
    assert again.rank == 50 and torch.equal(again.torch(), cpm.torch())
    assert again.to("cpu") is again
    with pytest.raises(AssertionError):
        tn.CPMatrix(cpm.cores, 7, [11, 3], [23, 2])                 # a rank that contradicts the cores


def test_ttmatrix_construction_then_product():
    """tests/test_matrix.py `test_tt_multiply` of the reference: a full-rank TTMatrix times a batch is v @ M."""
    torch.manual_seed(1)
    M = torch.rand(33, 46, dtype=torch.float64)
    v = torch.rand(30, 33, dtype=torch.float64)
    ttm = tn.TTMatrix(M, [50], [11, 3], [23, 2])
    assert torch.allclose(tn.tt_multiply(ttm, v), v @ M)


def test_refusals():
    ttm, cpm, x = _matrices("three", torch.float64)
    for mul, mat in ((tn.tt_multiply, ttm), (tn.cp_multiply, cpm)):
        with pytest.raises(ValueError, match="2 dimensions"):
            mul(mat, x[0])
        with pytest.raises(ValueError, match="multiple"):
            mul(mat, torch.zeros(3, 59, dtype=torch.float64))
        with pytest.raises(ValueError, match="float32 or float64"):
            mul(mat, torch.zeros(3, 60, dtype=torch.int64))
        with pytest.raises(ValueError, match="float32 or float64"):
            mul(mat, torch.zeros(3, 60, dtype=torch.float16))
        with pytest.raises(ValueError, match="same dtype"):
            mul(mat, x.float())
        with pytest.raises(ValueError, match="same device"):
            mul(mat, x.to("meta"))
        with pytest.raises(ValueError, match="first argument"):
            mul(mat.cores, x)
    with pytest.raises(ValueError, match="first argument"):
        tn.tt_multiply(cpm, x)
    with pytest.raises(ValueError, match="first argument"):
        tn.cp_multiply(ttm, x)
    batched = tn.TTMatrix([c[None].repeat(2, 1, 1, 1, 1) for c in ttm.cores], None, [4, 3, 5], [2, 6, 3])
    assert batched.batch
    with pytest.raises(ValueError, match="batched"):
        tn.tt_multiply(batched, x)
    g = torch.Generator().manual_seed(2)
    open_left = tn.TTMatrix([torch.randn((2, 4, 2, 3), dtype=torch.float64, generator=g), torch.randn((3, 3, 6, 1), dtype=torch.float64, generator=g)],
                            None, [4, 3], [2, 6])
    with pytest.raises(ValueError, match="boundary ranks"):
        tn.tt_multiply(open_left, torch.zeros(2, 12, dtype=torch.float64))
    open_right = tn.TTMatrix([torch.randn((1, 4, 2, 3), dtype=torch.float64, generator=g), torch.randn((3, 3, 6, 2), dtype=torch.float64, generator=g)],
                             None, [4, 3], [2, 6])
    with pytest.raises(ValueError, match="boundary ranks"):
        tn.tt_multiply(open_right, torch.zeros(2, 12, dtype=torch.float64))


@pytest.mark.parametrize("dt", DTYPES)
def test_empty_batch(dt):
    ttm, cpm, _ = _matrices("three", dt)
    for y in (tn.tt_multiply(ttm, torch.zeros((0, 60), dtype=dt)), tn.cp_multiply(cpm, torch.zeros((0, 4, 3, 5), dtype=dt))):
        assert tuple(y.shape) == (0, 36) and y.dtype == dt


def test_names_are_wired_through_every_layer():
    from tntorch_amd import _hip, _hipops, _hostops

    assert tn.matrix.__all__ == ["TTMatrix", "CPMatrix", "tt_multiply", "cp_multiply"]
    for name in tn.matrix.__all__:
        assert getattr(tn, name) is getattr(tn.matrix, name)
    with open(os.path.join(ROOT, "include", "ttround_hip.h")) as f:
        header = f.read()
    for name in ("ttr_ttm_step", "ttr_cpm_step"):
        assert re.search(r"\bint\s+{}\s*\(".format(name), header) and name in _hip.EXPORTED_SYMBOLS
    assert _hip.ABI_VERSION == 17
    assert re.search(r"ttr_ttm_step / ttr_cpm_step were ADDED\s+under 17", header)
    for mod in (_hipops, _hostops):
        assert callable(mod.tt_matvec_chain) and callable(mod.cp_matvec_chain)
    assert callable(_hip.ttm_step) and callable(_hip.cpm_step)
    with open(os.path.join(ROOT, "tntorch_amd", "csrc", "Makefile")) as f:
        assert "ttr_ttmatrix.hip" in f.read()
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        assert re.search(r"^## 24\.", f.read(), flags=re.M)
    with open(os.path.join(ROOT, "tools", "README.md")) as f:
        text = f.read()
    assert "gen_matrix_golden.py" in text and "ttmatrix_bench.py" in text
    assert "tt_multiply" in tn.__doc__ and "CPMatrix" in tn.__doc__

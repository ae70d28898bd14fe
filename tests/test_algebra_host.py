"""``tn.tt_apply`` / ``tn.tt_matmul`` / ``tn.tt_transpose`` on CPU tensors and the host mirror ``_hostops.core_compose``: against
fp64 contractions that are independent of the package (algebra_cases), ``tn.tt_multiply``, autograd through the dense product,
every refusal, the refusals of the C ABI (validation precedes any HIP call) and the wiring."""
import ctypes
import os
import re

import pytest
import torch

import algebra_cases as ac
import matrix_cases as mc
import tntorch_amd as tn
from tntorch_amd import _hip, _hipops, _hostops

F32, F64 = torch.float32, torch.float64
DTYPES = [F32, F64]


def _matrix(G, idims, odims):
    return tn.TTMatrix(list(G), None, idims, odims)


# ---------------------------------------------------------------------------------------------- the mirror
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", ac.SHAPES)
def test_mirror_one_core(shape, dt):
    A, B = ac.operands(shape, dt)
    out = _hostops.core_compose(A, B)
    R1, P, J, R2, S1, Q, S2 = shape
    assert out.dtype == dt and tuple(out.shape) == (R1 * S1, P, Q, R2 * S2)
    ref, bound = ac.core_truth_and_bound(A, B, dt)
    mc.assert_within(out, ref, bound, "mirror {} {}".format(shape, dt))


def test_mirror_is_the_formula_as_written():
    A, B = ac.operands((2, 3, 4, 3, 2, 2, 5), F64)
    out = _hostops.core_compose(A, B)
    for (r, a, p, q, s, b) in [(0, 0, 0, 0, 0, 0), (1, 0, 2, 1, 2, 4), (1, 1, 1, 0, 0, 3), (0, 1, 2, 1, 1, 0)]:
        want = sum(float(A[r, p, j, s]) * float(B[a, j, q, b]) for j in range(4))
        assert abs(float(out[r * 2 + a, p, q, s * 5 + b]) - want) <= 1e-14 * max(1.0, abs(want))


def test_mirror_refusals():
    A, B = ac.operands((2, 3, 4, 3, 2, 2, 5), F64)
    with pytest.raises(ValueError, match="4-d cores of one dtype"):
        _hostops.core_compose(A[0], B)
    with pytest.raises(ValueError, match="4-d cores of one dtype"):
        _hostops.core_compose(A, B.float())
    with pytest.raises(ValueError, match="the same J"):
        _hostops.core_compose(A, B[:, :3])


# ---------------------------------------------------------------------------------------------- products against the truth
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", ac.CASES)
def test_products_against_the_truth(name, dt):
    G, T, U, idims, odims = ac.case(name, dt)
    M = _matrix(G, idims, odims)
    y = tn.tt_apply(M, tn.Tensor(T))
    assert isinstance(y, tn.Tensor) and tuple(y.shape) == tuple(odims) and y.cores[0].dtype == dt
    y64, bound = ac.apply_truth_and_bound(G, T, dt)
    mc.assert_within(y.torch().reshape(-1), y64, bound, "tt_apply {} {}".format(name, dt))

    z = tn.tt_apply(M, tn.Tensor(U), transpose=True)
    assert tuple(z.shape) == tuple(idims) and z.cores[0].dtype == dt
    z64, bound = ac.apply_truth_and_bound(G, U, dt, transpose=True)
    mc.assert_within(z.torch().reshape(-1), z64, bound, "tt_apply transpose {} {}".format(name, dt))

    MT = tn.tt_transpose(M)
    P = tn.tt_matmul(M, MT)
    assert isinstance(P, tn.TTMatrix) and P.input_dims.tolist() == list(idims) and P.output_dims.tolist() == list(idims)
    p64, bound = ac.matmul_truth_and_bound(G, ac.transposed(G), dt)
    mc.assert_within(P.torch(), p64, bound, "tt_matmul {} {}".format(name, dt))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", ac.CASES)
def test_agrees_with_tt_multiply(name, dt):
    """Both are within their derived bound of the same truth, so within the sum of the two bounds of each other."""
    G, T, _, idims, odims = ac.case(name, dt)
    M, t = _matrix(G, idims, odims), tn.Tensor(T)
    got = tn.tt_apply(M, t).torch().reshape(-1)
    x = t.torch().reshape(1, -1)
    want = tn.tt_multiply(M, x)[0]
    y64, b1 = ac.apply_truth_and_bound(G, T, dt)
    _, b2 = mc.tt_truth_and_bound(G, x, dt)
    # (tt_multiply starts from the train's decompressed vector, itself rounded: its chain bound on |x| covers the product, the
    # decompression adds the train's own chain, which b1 already counts)
    mc.assert_within(got, want.double(), b1 + b2[0] + b1, "tt_apply against tt_multiply {} {}".format(name, dt))


def test_transpose_is_a_view_with_swapped_dims():
    G, _, _, idims, odims = ac.case("three", F64)
    M = _matrix(G, idims, odims)
    MT = tn.tt_transpose(M)
    assert MT.input_dims.tolist() == list(odims) and MT.output_dims.tolist() == list(idims)
    for a, b in zip(M.cores, MT.cores):
        assert b.data_ptr() == a.data_ptr() and tuple(b.shape) == (a.shape[0], a.shape[2], a.shape[1], a.shape[3])
    assert torch.equal(MT.torch(), M.torch().T)
    assert M.input_dims.tolist() == list(idims)


def test_unrounded_ranks_are_the_products():
    G, T, U, idims, odims = ac.case("three", F64)       # matrix ranks [7, 5], train ranks [3, 2]
    M = _matrix(G, idims, odims)
    assert tn.tt_apply(M, tn.Tensor(T)).ranks_tt.tolist() == [1, 21, 10, 1]
    assert tn.tt_apply(M, tn.Tensor(U), transpose=True).ranks_tt.tolist() == [1, 21, 10, 1]
    assert [c.shape[-1] for c in tn.tt_matmul(M, tn.tt_transpose(M)).cores] == [49, 25, 1]
    # the first factor of the product is major: train-major for the default, matrix-major for transpose
    y = tn.tt_apply(M, tn.Tensor(T)).cores[0]           # [1, O, 3 * 7]
    want = torch.einsum("njb,ajqs->nqbs", T[0], G[0]).reshape(1, odims[0], 21)
    assert torch.allclose(y, want, rtol=0, atol=1e-13)
    z = tn.tt_apply(M, tn.Tensor(U), transpose=True).cores[0]   # [1, I, 7 * 3]
    want = torch.einsum("rpjs,ajb->rapsb", G[0], U[0]).reshape(1, idims[0], 21)
    assert torch.allclose(z, want, rtol=0, atol=1e-13)


@pytest.mark.parametrize("dt", DTYPES)
def test_identity_operator_returns_the_cores_bit_for_bit(dt):
    dims = [4, 3, 5]
    T = ac.train_cores(dims, [3, 2], dt)
    eye = _matrix([torch.eye(n, dtype=dt).reshape(1, n, n, 1) for n in dims], dims, dims)
    for transpose in (False, True):
        out = tn.tt_apply(eye, tn.Tensor(T), transpose=transpose)
        for a, b in zip(out.cores, T):
            assert torch.equal(a, b)
    assert all(torch.equal(a, b) for a, b in zip(tn.tt_apply(eye, tn.Tensor(T), eps=1e-3).cores, T))   # rank 1: not rounded


def test_train_with_a_tucker_factor():
    G, T, _, idims, odims = ac.case("three", F64)
    g = torch.Generator().manual_seed(4)
    U1 = torch.randn(idims[1], 2, dtype=F64, generator=g)
    small = [T[0], torch.randn(3, 2, 2, dtype=F64, generator=g), T[2]]
    t = tn.Tensor(list(small), Us=[None, U1, None])
    assert tuple(t.shape) == tuple(idims)
    flat = [small[0], torch.einsum("asb,ns->anb", small[1], U1), small[2]]
    out = tn.tt_apply(_matrix(G, idims, odims), t)
    assert all(U is None for U in out.Us)
    y64, bound = ac.apply_truth_and_bound(G, flat, F64)
    mc.assert_within(out.torch().reshape(-1), y64, 2 * bound, "tucker factor")   # + the contraction of the factor


# ---------------------------------------------------------------------------------------------- rounding
def test_rounded_fp64_eps():
    """round_tt(eps) bounds the relative Frobenius error; the exact path adds its own 1e-12 (as for convolve)."""
    G, T, U, idims, odims = ac.case("three", F64)
    M = _matrix(G, idims, odims)
    y64, _ = ac.apply_truth_and_bound(G, T, F64)
    out = tn.tt_apply(M, tn.Tensor(T), eps=1e-6)
    err = ac.rel_err(out.torch().reshape(-1).numpy(), y64.numpy())
    print("tt_apply eps = 1e-6: relative error", err, "ranks", out.ranks_tt.tolist())
    assert err <= 1e-6 + 1e-12
    z64, _ = ac.apply_truth_and_bound(G, U, F64, transpose=True)
    out = tn.tt_apply(M, tn.Tensor(U), transpose=True, eps=1e-6, algorithm="eig")
    assert ac.rel_err(out.torch().reshape(-1).numpy(), z64.numpy()) <= 1e-6 + 1e-12
    p64, _ = ac.matmul_truth_and_bound(G, ac.transposed(G), F64)
    P = tn.tt_matmul(M, tn.tt_transpose(M), eps=1e-6)
    err = ac.rel_err(P.torch().numpy(), p64.numpy())
    print("tt_matmul eps = 1e-6: relative error", err, "ranks", [c.shape[-1] for c in P.cores])
    assert err <= 1e-6 + 1e-12
    assert [c.shape[-1] for c in P.cores][0] <= 16      # 4 x 4 rows of the first unfolding: the product rank 49 came down
    assert all(c.dim() == 4 for c in P.cores) and P.input_dims.tolist() == list(idims)


def test_rmax_caps_the_ranks():
    G, T, U, idims, odims = ac.case("three", F32)
    M = _matrix(G, idims, odims)
    assert tn.tt_apply(M, tn.Tensor(U), transpose=True, rmax=4).ranks_tt.tolist() == [1, 4, 4, 1]   # from [1, 21, 10, 1]
    assert tn.tt_apply(M, tn.Tensor(T), eps=None, rmax=2).ranks_tt.tolist() == [1, 2, 2, 1]
    assert [c.shape[-1] for c in tn.tt_matmul(M, tn.tt_transpose(M), rmax=5).cores] == [5, 5, 1]


def test_rank_one_operand_is_not_rounded_without_rmax(monkeypatch):
    G, T, _, idims, odims = ac.case("kron", F64)        # matrix ranks [1, 1]
    M = _matrix(G, idims, odims)
    G3, T3 = ac.case("three", F64)[:2]
    one = ac.train_cores(mc.RANDOM_CASES["three"][0], [1, 1], F64)

    def no_rounding(self, *args, **kwargs):
        raise AssertionError("round_tt ran")

    monkeypatch.setattr(tn.Tensor, "round_tt", no_rounding)
    assert tn.tt_apply(M, tn.Tensor(T), eps=1e-6).ranks_tt.tolist() == [1, 2, 3, 1]
    M3 = _matrix(G3, *mc.RANDOM_CASES["three"][:2])
    assert tn.tt_apply(M3, tn.Tensor(one), eps=1e-6).ranks_tt.tolist() == [1, 7, 5, 1]
    assert [c.shape[-1] for c in tn.tt_matmul(M, tn.tt_transpose(M), eps=1e-6).cores] == [1, 1, 1]
    with pytest.raises(AssertionError, match="round_tt ran"):
        tn.tt_apply(M, tn.Tensor(T), rmax=2)
    with pytest.raises(AssertionError, match="round_tt ran"):
        tn.tt_apply(M3, tn.Tensor(T3), eps=1e-6)


def test_inputs_are_unchanged():
    G, T, U, idims, odims = ac.case("three", F64)
    M, t = _matrix(G, idims, odims), tn.Tensor(T)
    g0, t0 = [c.clone() for c in M.cores], [c.clone() for c in t.cores]
    tn.tt_apply(M, t, eps=1e-6)
    tn.tt_apply(M, tn.Tensor(U), transpose=True, rmax=3)
    tn.tt_matmul(M, tn.tt_transpose(M), rmax=4)
    assert all(torch.equal(a, b) for a, b in zip(M.cores, g0)) and all(torch.equal(a, b) for a, b in zip(t.cores, t0))
    assert t.ranks_tt.tolist() == [1, 3, 2, 1] and M.input_dims.tolist() == list(idims) and M.output_dims.tolist() == list(odims)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals():
    G, T, U, idims, odims = ac.case("three", F64)
    M, t = _matrix(G, idims, odims), tn.Tensor(T)
    with pytest.raises(ValueError, match="tt_apply: the first argument must be a TTMatrix, got Tensor"):
        tn.tt_apply(t, t)
    with pytest.raises(ValueError, match="tt_apply: t must be a tntorch_amd.Tensor, got Tensor"):
        tn.tt_apply(M, t.torch())
    with pytest.raises(ValueError, match="tt_matmul: the second argument must be a TTMatrix"):
        tn.tt_matmul(M, t)
    with pytest.raises(ValueError, match="tt_matmul: the first argument must be a TTMatrix"):
        tn.tt_matmul(M.torch(), M)
    with pytest.raises(ValueError, match="tt_transpose: the argument must be a TTMatrix"):
        tn.tt_transpose(t)
    batched_m = tn.TTMatrix([g[None].expand(2, -1, -1, -1, -1) for g in G], None, idims, odims)
    with pytest.raises(ValueError, match=r"tt_apply: batched matrices \(5-D cores\) are not supported"):
        tn.tt_apply(batched_m, t)
    with pytest.raises(ValueError, match="tt_matmul: batched matrices"):
        tn.tt_matmul(M, batched_m)
    with pytest.raises(ValueError, match="tt_transpose: batched matrices"):
        tn.tt_transpose(batched_m)
    batched_t = tn.Tensor([c[None].expand(2, -1, -1, -1).contiguous() for c in T], batch=True)
    with pytest.raises(ValueError, match="tt_apply: batched tensors are not supported"):
        tn.tt_apply(M, batched_t)
    open_m = _matrix([G[0].expand(2, -1, -1, -1)] + G[1:], idims, odims)
    with pytest.raises(ValueError, match="tt_apply: the boundary ranks must be 1, got 2 and 1"):
        tn.tt_apply(open_m, t)
    with pytest.raises(ValueError, match="tt_matmul: the boundary ranks must be 1, got 2 and 1"):
        tn.tt_matmul(open_m, tn.tt_transpose(M))
    with pytest.raises(ValueError, match="tt_apply: the matrix has 3 modes, the tensor 2"):
        tn.tt_apply(M, tn.Tensor(ac.train_cores(idims[:2], [2], F64)))
    with pytest.raises(ValueError, match="tt_apply: mode 0 of the tensor has size 2, the matrix's input mode 4"):
        tn.tt_apply(M, tn.Tensor(U))                      # a train over output_dims without transpose
    with pytest.raises(ValueError, match="tt_apply: mode 0 of the tensor has size 4, the matrix's output mode 2"):
        tn.tt_apply(M, t, transpose=True)
    two = _matrix(G[:1] + [G[1][..., :1]], idims[:2], odims[:2])
    with pytest.raises(ValueError, match="tt_matmul: the matrices have 3 and 2 modes"):
        tn.tt_matmul(M, two)
    with pytest.raises(ValueError, match="tt_matmul: mode 0: the first matrix's output mode has size 2, the second's input mode 4"):
        tn.tt_matmul(M, M)
    half = _matrix([g.half() for g in G], idims, odims)
    with pytest.raises(ValueError, match="tt_apply: float32 or float64 operands are needed, got torch.float16"):
        tn.tt_apply(half, tn.Tensor([c.half() for c in T]))
    with pytest.raises(ValueError, match="tt_apply: the operands must have the same dtype"):
        tn.tt_apply(M, tn.Tensor([c.float() for c in T]))
    with pytest.raises(ValueError, match="tt_matmul: the operands must have the same dtype"):
        tn.tt_matmul(M, tn.tt_transpose(_matrix([g.float() for g in G], idims, odims)))
    meta = tn.Tensor([c.to("meta") for c in T])
    with pytest.raises(ValueError, match="tt_apply: the operands must be on the same device"):
        tn.tt_apply(M, meta)
    with pytest.raises(ValueError, match="tt_matmul: the operands must be on the same device"):
        tn.tt_matmul(M, _matrix([g.to("meta") for g in ac.transposed(G)], odims, idims))
    cp = tn.Tensor([torch.rand(n, 2, dtype=F64) for n in idims])
    with pytest.raises(NotImplementedError, match="tt_apply of CP cores"):
        tn.tt_apply(M, cp)


# ---------------------------------------------------------------------------------------------- CPU gradients
def test_cpu_gradients_against_autograd_through_the_dense_product():
    """The chain is plain torch on the CPU.  fp64: both sides are sums of at most a few thousand products of O(1) numbers, so
    1e-10 of the largest entry is orders above their rounding (the reasoning of test_lookup_host.py)."""
    G, T, U, idims, odims = ac.case("three", F64)
    g = torch.Generator().manual_seed(9)
    w = torch.randn(int(torch.tensor(odims).prod()), dtype=F64, generator=g)

    def leaves(xs):
        return [x.clone().requires_grad_(True) for x in xs]

    def dense_loss(Gs, Ts):
        acc = None
        for c in Ts:
            acc = c if acc is None else torch.einsum("anb,bmc->anmc", acc, c).reshape(acc.shape[0], -1, c.shape[2])
        M = None
        for c in Gs:
            M = c if M is None else torch.einsum("aiob,bjpc->aijopc", M, c).reshape(M.shape[0], M.shape[1] * c.shape[1], M.shape[2] * c.shape[2], c.shape[3])
        return ((acc[0, :, 0] @ M[0, :, :, 0]) * w).sum()

    Ga, Ta = leaves(G), leaves(T)
    loss = (tn.tt_apply(_matrix(Ga, idims, odims), tn.Tensor(Ta)).torch().reshape(-1) * w).sum()
    got = torch.autograd.grad(loss, Ga + Ta)
    Gb, Tb = leaves(G), leaves(T)
    want = torch.autograd.grad(dense_loss(Gb, Tb), Gb + Tb)
    for a, b in zip(got, want):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-10 * float(b.abs().max())

    # tt_matmul: gradients of both matrices' cores through trace-like weights on the dense product
    Ga, Gb = leaves(G), leaves(ac.transposed(G))
    W = torch.randn(mc.tt_dense(G).shape[0], mc.tt_dense(G).shape[0], dtype=F64, generator=g)
    loss = (tn.tt_matmul(_matrix(Ga, idims, odims), _matrix(Gb, odims, idims)).torch() * W).sum()
    got = torch.autograd.grad(loss, Ga + Gb)

    def dense_m(Gs):
        M = None
        for c in Gs:
            M = c if M is None else torch.einsum("aiob,bjpc->aijopc", M, c).reshape(M.shape[0], M.shape[1] * c.shape[1], M.shape[2] * c.shape[2], c.shape[3])
        return M[0, :, :, 0]

    Gc, Gd = leaves(G), leaves(ac.transposed(G))
    want = torch.autograd.grad(((dense_m(Gc) @ dense_m(Gd)) * W).sum(), Gc + Gd)
    for a, b in zip(got, want):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-10 * float(b.abs().max())


# ---------------------------------------------------------------------------------------------- the C ABI's refusals
F32C, F64C = 0, 1
INVALID, UNSUPPORTED = -1, -2
_BUF = [(ctypes.c_double * 512)() for _ in range(3)]
A0, A1, A2 = (ctypes.addressof(b) for b in _BUF)


def compose(dtype=F32C, R1=2, P=3, J=4, R2=3, S1=2, Q=2, S2=5, A=A0, B=A1, out=A2):
    return dtype, R1, P, J, R2, S1, Q, S2, A, B, out, None


REFUSALS = [
    (compose(dtype=7), INVALID, "ttr_core_compose: bad dtype 7"),
    (compose(dtype=-1), INVALID, "ttr_core_compose: bad dtype -1"),
] + [
    (compose(**{name: 0}), INVALID, "ttr_core_compose: bad sizes") for name in ("R1", "P", "J", "R2", "S1", "Q", "S2")
] + [
    (compose(Q=-3), INVALID, "ttr_core_compose: bad sizes [2, 3, 4, 3] x [2, 4, -3, 5]"),
    (compose(A=None), INVALID, "ttr_core_compose: null pointer"),
    (compose(B=None), INVALID, "ttr_core_compose: null pointer"),
    (compose(out=None), INVALID, "ttr_core_compose: null pointer"),
    (compose(out=A0), INVALID, "ttr_core_compose: out must not be an input"),
    (compose(out=A1), INVALID, "ttr_core_compose: out must not be an input"),
    (compose(J=1 << 31), UNSUPPORTED, "ttr_core_compose: an extent does not fit 32 bits"),
    (compose(P=1 << 31), UNSUPPORTED, "ttr_core_compose: an extent does not fit 32 bits"),
    (compose(R1=1 << 16, S1=1 << 16), UNSUPPORTED, "ttr_core_compose: a rank product does not fit 32 bits"),
    (compose(R2=1 << 20, S2=1 << 11), UNSUPPORTED, "ttr_core_compose: a rank product does not fit 32 bits"),
    (compose(R1=1 << 15, P=1 << 15, J=1 << 15, R2=1 << 15, S1=1, Q=1, S2=1), UNSUPPORTED, "ttr_core_compose: operand too large"),
    (compose(R1=1 << 15, P=1 << 14, J=1, R2=1 << 15, S1=1 << 15, Q=1, S2=1 << 15), UNSUPPORTED, "ttr_core_compose: operand too large"),
    # 2^24 x 2^20 tiles of a result of 2^56 elements
    (compose(R1=1 << 15, P=1 << 15, J=1, R2=1, S1=1 << 15, Q=1 << 11, S2=1), UNSUPPORTED, "workgroups do not fit a 32-bit grid"),
]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()  # hipcc cross-compiles gfx950 without a GPU
    L = ctypes.CDLL(g.LIB)
    for name, (res, args) in _hip._SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L


@pytest.mark.skipif(torch.cuda.is_available(), reason="host addresses must not reach a launch on a real device")
@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_cabi_refusal(lib, case):
    """The checks return before anything touches a device: the library is called with the addresses of small host arrays."""
    args, status, text = REFUSALS[case]
    assert lib.ttr_core_compose(*args) == status
    assert text in lib.ttr_last_error().decode()


# ---------------------------------------------------------------------------------------------- wiring
def test_wiring():
    root = mc.ROOT
    assert tn.ttalgebra.__all__ == ["tt_apply", "tt_matmul", "tt_transpose"]
    assert tn.tt_apply is tn.ttalgebra.tt_apply and tn.tt_matmul is tn.ttalgebra.tt_matmul and tn.tt_transpose is tn.ttalgebra.tt_transpose
    assert tn.matrix.__all__ == ["TTMatrix", "CPMatrix", "tt_multiply", "cp_multiply"]
    header = open(os.path.join(root, "include", "ttround_hip.h")).read()
    above, below = header.split("#define TTR_ABI_VERSION")
    assert "ttr_core_compose" in above
    assert re.search(r"\bint\s+ttr_core_compose\s*\(\s*int dtype, int64_t R1, int64_t P, int64_t J, int64_t R2, int64_t S1, int64_t Q,\s*"
                     r"int64_t S2,\s*const void\* A,\s*const void\* B, void\* out, void\* stream\)", below)
    assert _hip.ABI_VERSION == 17
    assert "ttr_core_compose" in _hip.EXPORTED_SYMBOLS
    assert (_hip.COMPOSE_TILE_M, _hip.COMPOSE_TILE_N, _hip.COMPOSE_TILE_K) == (ac.TILE_M, ac.TILE_N, ac.TILE_K)
    assert _hip.COMPOSE_TILE_M >= 16 and _hip.COMPOSE_TILE_N >= 16 and _hip.COMPOSE_TILE_K % 4 == 0
    makefile = open(os.path.join(root, "tntorch_amd", "csrc", "Makefile")).read()
    assert re.search(r"^  ttr_ttcompose\.hip \\$", makefile, flags=re.M)
    assert os.path.exists(os.path.join(root, "tntorch_amd", "csrc", "ttr_ttcompose.hip"))
    assert callable(_hipops.core_compose) and callable(_hostops.core_compose) and callable(_hip.core_compose)
    assert "## 28." in open(os.path.join(root, "DESIGN.md")).read()

"""ttr_core_matvec and ttr_hsum_step through the C ABI on a real MI355X, against torch.einsum in fp64 on the CPU, with the
tolerances tests/test_gpu_kernels.py uses for ttr_gemm (5e-6 / 1e-12 of the largest entry).  Shapes: nothing a tile multiple, K = 1
and one past an MFMA k-step multiple, both sides of a 16-wide tile edge, single rows / columns, more than one batch item."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DT = [torch.float32, torch.float64]


def tol(dt, f32=5e-6, f64=1e-12):
    return f32 if dt == torch.float32 else f64


def _hip():
    from tntorch_amd import _hip

    _hip.lib()
    return _hip


def _i64(v):
    return (ctypes.c_int64 * len(v))(*[int(x) for x in v])


MATVEC_SHAPES = [
    (3, 5, 2, 4, 7, 3),     # nothing a tile multiple
    (3, 1, 2, 4, 7, 3),     # K = 1
    (3, 17, 2, 4, 7, 3),    # K one past an MFMA k-step multiple
    (3, 5, 2, 4, 1, 3),     # S = 1
    (3, 5, 3, 5, 2, 5),     # P A = 15, Q C = 15
    (4, 5, 2, 4, 2, 8),     # P A = 16, Q C = 16
    (1, 5, 17, 17, 2, 1),   # P A = 17, Q C = 17
    (1, 6, 1, 9, 5, 11),    # P = Q = 1: the first step of the chain
    (2, 16, 40, 3, 2, 50),  # several tiles in both directions (Q = 40 rows, A C = 150 columns)
]


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("P,K,Q,A,S,C", MATVEC_SHAPES)
def test_core_matvec(dt, P, K, Q, A, S, C):
    h = _hip()
    g = torch.Generator().manual_seed(P * 1000 + K * 100 + Q * 10 + A + S + C)
    x = torch.randn(P, K, Q, generator=g, dtype=torch.float64).to(dt)
    G = torch.randn(A, K, S, C, generator=g, dtype=torch.float64).to(dt)
    ref = torch.einsum("pkq,aksc->pasqc", x.double(), G.double()).reshape(P * A, S, Q * C)
    out = h.core_matvec(x.cuda(), G.cuda())
    assert tuple(out.shape) == (P * A, S, Q * C) and out.is_contiguous()
    err = (out.cpu().double() - ref).abs().max() / ref.abs().max()
    assert err < tol(dt), err


@pytest.mark.parametrize("dt", DT)
def test_core_matvec_refuses_non_contiguous_operands(dt):
    h = _hip()
    L = h.lib()
    x = torch.randn(3, 5, 2, dtype=dt).cuda()
    G = torch.randn(4, 5, 7, 3, dtype=dt).cuda()
    out = torch.full((12, 7, 6), 7.0, dtype=dt).cuda()
    xt = torch.randn(3, 2, 5, dtype=dt).cuda().transpose(1, 2)       # [3, 5, 2] with strides (10, 1, 5)
    Gt = torch.randn(4, 5, 7, 6, dtype=dt).cuda()[..., ::2]           # [4, 5, 7, 3] with a column stride of 2
    code = h.dtype_code(dt)
    for xs, gs in ((xt.stride(), G.stride()), (x.stride(), Gt.stride())):
        rc = L.ttr_core_matvec(code, 3, 5, 2, 4, 7, 3, x.data_ptr(), _i64(xs), G.data_ptr(), _i64(gs), out.data_ptr(), None)
        assert rc == h.E_UNSUPPORTED and b"contiguous" in L.ttr_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())   # nothing was launched
    with pytest.raises(NotImplementedError, match="contiguous"):
        h.core_matvec(xt, G)
    # the strides of extent-1 axes are free
    x1 = torch.randn(1, 5, 1, dtype=dt).cuda()
    rc = L.ttr_core_matvec(code, 1, 5, 1, 4, 7, 3, x1.data_ptr(), _i64((99, 1, 77)), G.data_ptr(), _i64(G.stride()), out.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    ref = torch.einsum("pkq,aksc->pasqc", x1.cpu().double(), G.cpu().double()).reshape(4, 7, 3)
    assert (out.cpu().double().reshape(-1)[: 4 * 7 * 3].reshape(4, 7, 3) - ref).abs().max() / ref.abs().max() < tol(dt)
    assert L.ttr_core_matvec(code, 0, 5, 1, 4, 7, 3, x1.data_ptr(), _i64((5, 1, 1)), G.data_ptr(), _i64(G.stride()), out.data_ptr(), None) == h.E_INVALID


HSUM_CASES = [
    # I, r_in, r_out
    (5, [3], [4]),                        # K = 1
    (5, [3, 2], [2, 4]),                  # K = 2
    (5, [3, 2, 4], [2, 3, 2]),            # K = 3
    (5, [3, 2, 2, 3], [2, 3, 2, 2]),      # K = 4
    (6, [1, 1, 1], [1, 1, 1]),            # all ranks 1
    (7, [17, 3, 2], [2, 17, 3]),          # ranks (17, 3, 2)
    (1, [4, 3, 2], [3, 2, 5]),            # I = 1
    (33, [4, 3, 2], [3, 2, 5]),           # I = 33
    (9, [40, 20], [70, 35]),              # more than one tile of rows and of columns in the last mode, ragged
]


def _hsum_ref(W, cores):
    letters_in, letters_out = "abcd", "wxyz"
    K = len(cores)
    spec = letters_in[:K] + "," + ",".join(letters_in[m] + "i" + letters_out[m] for m in range(K)) + "->" + letters_out[:K]
    return torch.einsum(spec, W.double(), *[c.double() for c in cores])


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("I,rin,rout", HSUM_CASES)
def test_hsum_step(dt, I, rin, rout):
    h = _hip()
    g = torch.Generator().manual_seed(I * 100 + sum(rin) * 10 + sum(rout))
    W = torch.randn(rin, generator=g, dtype=torch.float64).to(dt)
    cores = [torch.randn(a, I, b, generator=g, dtype=torch.float64).to(dt) for a, b in zip(rin, rout)]
    ref = _hsum_ref(W, cores)
    out = h.hsum_step(W.cuda(), [c.cuda() for c in cores])
    assert list(out.shape) == rout
    err = (out.cpu().double() - ref).abs().max() / ref.abs().max()
    assert err < tol(dt), err


@pytest.mark.parametrize("dt", DT)
def test_hsum_chain_of_two_is_dot(dt):
    """K = 2: the chain of ttr_hsum_step over the modes gives what _hipops.dot gives."""
    from tntorch_amd import _hipops

    g = torch.Generator().manual_seed(5)
    ra, rb = [1, 4, 17, 3, 1], [1, 2, 5, 6, 1]
    shape = [5, 33, 7, 4]
    a = [torch.rand(ra[n], shape[n], ra[n + 1], generator=g, dtype=torch.float64).to(dt).cuda() for n in range(4)]
    b = [torch.rand(rb[n], shape[n], rb[n + 1], generator=g, dtype=torch.float64).to(dt).cuda() for n in range(4)]
    W = torch.ones(1, 1, dtype=dt).cuda()
    for n in range(4):
        W = _hipops.hsum_step(W, [a[n], b[n]])
    d = _hipops.dot([c[None] for c in a], [c[None] for c in b])
    assert W.numel() == 1 and d.dim() == 0
    assert abs(float(W) - float(d)) < tol(dt) * abs(float(d))


@pytest.mark.parametrize("dt", DT)
def test_hsum_step_refusals(dt):
    h = _hip()
    L = h.lib()
    code = h.dtype_code(dt)
    I, rin, rout = 5, [3, 2, 4], [2, 3, 2]
    W = torch.randn(rin, dtype=dt).cuda()
    cores = [torch.randn(a, I, b, dtype=dt).cuda() for a, b in zip(rin, rout)]
    out = torch.full(rout, 7.0, dtype=dt).cuda()
    need = h.hsum_step_workspace_bytes(dt, I, rin, rout)
    assert need == 2 * 512 * (1 if dt == torch.float32 else 2)   # 5 * max(2*2*4, 2*3*4) = 120 elements per half, 256-byte aligned
    ws = torch.zeros(need, dtype=torch.uint8).cuda()
    ptrs = (ctypes.c_void_p * 3)(*[c.data_ptr() for c in cores])
    strides = [s for c in cores for s in c.stride()]

    def call(strides, ws_ptr, ws_bytes):
        return L.ttr_hsum_step(code, 3, I, _i64(rin), _i64(rout), W.data_ptr(), ptrs, _i64(strides), out.data_ptr(), ws_ptr, ws_bytes, None)

    # a scratch one byte below the bound is refused, not used
    assert call(strides, ws.data_ptr(), need - 1) == h.E_WORKSPACE
    assert call(strides, None, need) == h.E_WORKSPACE
    # the strides of a transposed core (core 1 as [3, 5, 2] -> permuted view) are refused, not read
    bad = list(strides)
    bad[3:6] = [1, 2, 10]
    assert call(bad, ws.data_ptr(), need) == h.E_UNSUPPORTED and b"contiguous" in L.ttr_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 0).all())   # nothing was launched
    assert call(strides, ws.data_ptr(), need) == 0
    torch.cuda.synchronize()
    ref = _hsum_ref(W.cpu(), [c.cpu() for c in cores])
    assert (out.cpu().double() - ref).abs().max() / ref.abs().max() < tol(dt)
    with pytest.raises(NotImplementedError, match="contiguous"):
        h.hsum_step(W, [cores[0], torch.randn(3, I, 2, dtype=dt).cuda().permute(2, 1, 0), cores[2]])


def test_exact_algorithm_names_eig_when_the_scratch_is_too_large():
    """prod_m r_m beyond the entry's scratch limit: the Python layer raises ValueError naming algorithm="eig" (nothing is allocated:
    the cores are tiny expanded views)."""
    from tntorch_amd import _hipops

    base = torch.ones(1, dtype=torch.float32).cuda()
    cores = [base.expand(200, 64, 200) for _ in range(4)]     # the intermediates would hold 64 * 200^4 elements
    with pytest.raises(ValueError, match='algorithm="eig"'):
        _hipops.hsum_step(base.expand(200, 200, 200, 200), cores)

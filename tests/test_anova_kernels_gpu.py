"""ttr_mode_sandwich through the C ABI and its wrapper on a real MI355X, in both dtypes, against the fp64 einsum on the CPU.
Tolerance: 5e-6 (fp32) / 1e-12 (fp64) of the reference's largest entry, those of test_moments_kernels_gpu.py; a plain torch fp32
evaluation of the two contractions on the CPU stays at or below 2.1e-7 on these shapes.

Shapes (S, R, I, C), anova_cases.SANDWICH_SHAPES: nothing a multiple of the 16-tile, both sides of a 16 edge, the rank limit, I
below, at and above one chunk of 8 slices and many chunks, S > 1, and the I = 1 call that computes mu^T Z mu; each with w / mu
given and NULL."""
import ctypes

import pytest
import torch

import anova_cases as ac
from tntorch_amd import _hip as h
from tntorch_amd import _hipops

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
SENTINEL = 7.0


def _i64(values):
    return (ctypes.c_int64 * len(values))(*[int(v) for v in values])


def _check(Q, shape, given, dt, what):
    ref = ac.sandwich_reference(shape, given)
    assert Q.is_cuda and Q.dtype == dt and tuple(Q.shape) == tuple(ref.shape) and Q.is_contiguous()
    err = float((Q.cpu().double() - ref).abs().max() / ref.abs().max())
    print(what, shape, "given" if given else "null", dt, "rel. error", err)
    assert err < (5e-6 if dt == torch.float32 else 1e-12), (what, shape, given, err)


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("given", [True, False], ids=["w_mu", "null"])
@pytest.mark.parametrize("shape", ac.SANDWICH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mode_sandwich(shape, given, dt):
    Z, A, w, mu = (x.to(dt).cuda() for x in ac.sandwich_inputs(shape))
    args = (Z, A, w if given else None, mu if given else None)
    Q = h.mode_sandwich(*args)
    _check(Q, shape, given, dt, "fused")
    assert torch.equal(Q, h.mode_sandwich(*args))        # bit-identical from call to call
    if max(shape[1], shape[3]) <= _hipops.SANDWICH_FUSED_MAX_RANK:
        assert torch.equal(Q, _hipops.mode_sandwich(*args))  # what the package's op launches at these ranks
    else:
        _check(_hipops.mode_sandwich(*args), shape, given, dt, "op")
    Zc, Ac = (x.to(dt) for x in ac.sandwich_inputs(shape)[:2])
    assert torch.equal(Z.cpu(), Zc) and torch.equal(A.cpu(), Ac)   # the inputs are left alone


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("shape", [(3, 5, 7, 6), (2, 33, 40, 20)], ids=lambda s: "x".join(map(str, s)))
def test_hsum_route_agrees(shape, dt):
    """The route the package takes above the fused kernel's rank limit, at ranks both can do."""
    Z, A, w, mu = (x.to(dt).cuda() for x in ac.sandwich_inputs(shape))
    _check(_hipops.mode_sandwich_hsum(Z, A, w, mu), shape, True, dt, "hsum")
    _check(_hipops.mode_sandwich_hsum(Z, A, None, None), shape, False, dt, "hsum")


def test_workspace_follows_the_shape():
    """One chunk of i: no workspace; more: [S, nsplit, C C] elements, rounded up to 256 bytes.  Chunks are 8 slices until S times
    their number would pass 512 workgroups."""
    wsb = h.mode_sandwich_workspace_bytes
    assert wsb(torch.float32, 3, 5, 7, 6) == 0 and wsb(torch.float64, 2, 7, 8, 9) == 0 and wsb(torch.float32, 2, 5, 1, 6) == 0
    assert wsb(torch.float32, 2, 16, 9, 17) == 2 * 2 * 17 * 17 * 4 + 256 - (2 * 2 * 17 * 17 * 4) % 256
    assert wsb(torch.float64, 4, 20, 130, 31) == 4 * 17 * 31 * 31 * 8 + 256 - (4 * 17 * 31 * 31 * 8) % 256
    assert wsb(torch.float32, 1, 4, 8192, 4) == 512 * 16 * 4           # chunks of 16: 512 workgroups
    assert wsb(torch.float32, 1, 65, 7, 3) == h.E_UNSUPPORTED and wsb(torch.float32, 1, 3, 0, 3) == h.E_INVALID


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "fp64"])
def test_refusals_leave_the_output_untouched(dt):
    L = h.lib()
    code = h.dtype_code(dt)
    shape = (2, 16, 9, 17)                                 # two chunks: the call needs a workspace
    S, R, I, C = shape
    Z, A, w, mu = (x.to(dt).cuda() for x in ac.sandwich_inputs(shape))
    Q = torch.full((S, C, C), SENTINEL, dtype=dt).cuda()
    need = h.mode_sandwich_workspace_bytes(dt, S, R, I, C)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8).cuda()
    At = A.permute(2, 1, 0).contiguous().permute(2, 1, 0)  # [R, I, C] but not contiguous
    astr = _i64(A.stride())

    def call(S=S, R=R, I=I, C=C, z=Z, a=A, astr=astr, q=Q, wsp=ws, wsn=need, dtype=code):
        ptr = lambda x: None if x is None else x.data_ptr()
        return L.ttr_mode_sandwich(dtype, S, R, I, C, ptr(z), ptr(a), astr, w.data_ptr(), mu.data_ptr(), ptr(q), ptr(wsp), wsn, None)

    assert call(dtype=7) == h.E_INVALID
    assert call(S=0) == h.E_INVALID and call(R=0) == h.E_INVALID and call(I=-1) == h.E_INVALID and call(C=0) == h.E_INVALID
    assert call(z=None) == h.E_INVALID and call(a=None) == h.E_INVALID and call(astr=None) == h.E_INVALID
    assert call(q=None) == h.E_INVALID
    assert call(a=At, astr=_i64(At.stride())) == h.E_UNSUPPORTED
    assert call(astr=_i64((I * C + 1, C, 1))) == h.E_UNSUPPORTED
    assert call(wsn=need - 1) == h.E_WORKSPACE and call(wsp=None) == h.E_WORKSPACE and call(wsn=0) == h.E_WORKSPACE
    big = h.mode_sandwich_max_rank() + 1
    assert h.mode_sandwich_max_rank() >= 64
    assert call(R=big) == h.E_UNSUPPORTED and call(C=big) == h.E_UNSUPPORTED   # refused on the sizes alone, nothing is read
    torch.cuda.synchronize()
    assert bool((Q.cpu() == SENTINEL).all())
    with pytest.raises(NotImplementedError):
        h.mode_sandwich(Z, At, w, mu)
    with pytest.raises(NotImplementedError):
        h.mode_sandwich(torch.zeros(1, big, big, dtype=dt).cuda(), torch.zeros(big, 2, 3, dtype=dt).cuda())
    with pytest.raises(ValueError):
        h.mode_sandwich(Z, A, w[:4], mu)
    with pytest.raises(ValueError):
        h.mode_sandwich(Z, A, w, mu[:, :4])
    assert call() == 0                                     # and the same arguments without a fault go through
    _check(Q, shape, True, dt, "after the refusals")


def test_symbols_are_declared_and_exported():
    for name in ("ttr_mode_sandwich", "ttr_mode_sandwich_workspace_bytes", "ttr_mode_sandwich_max_rank"):
        assert name in h.EXPORTED_SYMBOLS and hasattr(h.lib(), name)

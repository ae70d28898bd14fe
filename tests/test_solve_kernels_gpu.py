"""ttr_env_half_apply through the C ABI on a real MI355X, fp32 and fp64, against the fp64 einsum of the same (rounded) inputs, and
the device ops built on it (``local_matvec``, ``env_update``).

Per element |H - H64| <= 2 (R' + A J + 2) u half_apply64(|Phi|, |X|, |G|) (solve_cases: derived, not measured).  The shapes
(solve_cases.SHAPES) put R and S' one below, at and one above the row tile, I A' at 15 / 16 / 17 and around the column tile, R' and
A J around one and two staged chunks, J and R' off the MFMA quads, every axis at 1, and several tiles on all three grid axes.
Beyond the values: exactly the output's elements are written (sentinel guards), the same call gives the same bits, strided views
of G and X give the bits of their contiguous copies, and an element's bits do not depend on where it lies in a tile or on the
other output extents."""
import ctypes
import functools

import pytest
import torch

import solve_cases as sc
from tntorch_amd import _hip as h
from tntorch_amd import _hipops

pytestmark = pytest.mark.gpu

DTYPES = sc.DTYPES
SENTINEL = -77.0
GUARD = 64


@functools.lru_cache(maxsize=None)
def _case(shape, dt):
    Phi, X, G = sc.operands(shape, dt)
    ref, bound = sc.half_truth_and_bound(Phi, X, G, dt)
    return Phi, X, G, ref, bound


def _i64(v):
    return (ctypes.c_int64 * len(v))(*[int(s) for s in v])


def _raw(L, dt, phi_t, x_t, g_t, out_ptr, **over):
    R, A, Rp = phi_t.shape
    _, J, Sp = x_t.shape
    _, I, _, Ap = g_t.shape
    a = dict(dtype=h.dtype_code(dt), R=R, A=A, Rp=Rp, J=J, Sp=Sp, I=I, Ap=Ap, Phi=phi_t.data_ptr(), X=x_t.data_ptr(),
             xs=_i64(x_t.stride()), G=g_t.data_ptr(), gs=_i64(g_t.stride()), H=out_ptr)
    a.update(over)
    return L.ttr_env_half_apply(a["dtype"], a["R"], a["A"], a["Rp"], a["J"], a["Sp"], a["I"], a["Ap"], a["Phi"], a["X"], a["xs"],
                                a["G"], a["gs"], a["H"], None)


def test_tile_extents():
    assert (h.ENV_TILE_R, h.ENV_TILE_S, h.ENV_TILE_N, h.ENV_TILE_K) == (16, 16, 64, 16)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", sc.SHAPES)
def test_env_half_apply(shape, dt):
    """The output lies in a sentinel-filled buffer with guards before and after it: every element of H is written (a sentinel left
    behind breaks the bound), the guards stay as they were, a second call gives the same bits, and so does the wrapper."""
    L = h.lib()
    Phi, X, G, ref, bound = _case(shape, dt)
    Pd, Xd, Gd = Phi.cuda(), X.cuda(), G.cuda()
    item, n = Pd.element_size(), ref.numel()
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=dt, device="cuda")
    assert _raw(L, dt, Pd, Xd, Gd, buf.data_ptr() + GUARD * item) == 0, L.ttr_last_error()
    first = buf.cpu()
    assert bool((first[:GUARD] == SENTINEL).all()) and bool((first[GUARD + n:] == SENTINEL).all())
    sc.assert_within(first[GUARD:GUARD + n].reshape(ref.shape), ref, bound, "env_half_apply {} {}".format(shape, dt))
    assert _raw(L, dt, Pd, Xd, Gd, buf.data_ptr() + GUARD * item) == 0
    assert torch.equal(buf.cpu(), first)
    fresh = h.env_half_apply(Pd, Xd, Gd)
    assert fresh.shape == ref.shape and torch.equal(fresh.cpu().reshape(-1), first[GUARD:GUARD + n])
    assert torch.equal(Pd.cpu(), Phi) and torch.equal(Xd.cpu(), X) and torch.equal(Gd.cpu(), G)


@pytest.mark.parametrize("dt", DTYPES)
def test_layout_with_exact_data(dt):
    """Small integers: every product and sum is exact, so a swapped index shows as a wrong integer, not as rounding."""
    g = torch.Generator().manual_seed(3)
    R, A, Rp, J, Sp, I, Ap = 18, 2, 5, 3, 19, 7, 11
    Phi = torch.randint(-3, 4, (R, A, Rp), generator=g).to(dt)
    X = torch.randint(-3, 4, (Rp, J, Sp), generator=g).to(dt)
    G = torch.randint(-3, 4, (A, I, J, Ap), generator=g).to(dt)
    assert torch.equal(h.env_half_apply(Phi.cuda(), X.cuda(), G.cuda()).cpu().double(), sc.half_apply64(Phi, X, G))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", [(5, 2, 7, 3, 6, 3, 2), (17, 2, 2, 2, 15, 2, 3), (3, 1, 31, 31, 5, 2, 3)])
def test_strided_views_give_the_bits_of_their_copies(shape, dt):
    """G as a tt_transpose view ([a, j, i, c] storage) and as the rank-swapped view of the right-to-left sweep ([c, i, j, a]
    storage), X as the mirrored view ([s, j, b] storage): read where they lie, same bits as the contiguous copies."""
    Phi, X, G, ref, bound = _case(shape, dt)
    Pd, Xd, Gd = Phi.cuda(), X.cuda(), G.cuda()
    want = h.env_half_apply(Pd, Xd, Gd)
    Gt = Gd.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    Gs = Gd.permute(3, 1, 2, 0).contiguous().permute(3, 1, 2, 0)
    Xm = Xd.permute(2, 1, 0).contiguous().permute(2, 1, 0)
    assert not Gt.is_contiguous() or min(G.shape[1:3]) == 1
    for name, got in (("transposed G", h.env_half_apply(Pd, Xd, Gt)), ("rank-swapped G", h.env_half_apply(Pd, Xd, Gs)),
                      ("mirrored X", h.env_half_apply(Pd, Xm, Gd)), ("all", h.env_half_apply(Pd, Xm, Gs))):
        assert torch.equal(got, want), name
    sc.assert_within(want, ref, bound, "strided {} {}".format(shape, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_a_block_of_a_large_output_has_the_bits_of_the_sliced_operands(dt):
    """An element is one chain fixed by R', A, J and the dtype: slicing r, i, a' or s' of the operands (another place in the tiles,
    other output extents, strided views of G and X) leaves the bits."""
    shape = (33, 2, 9, 6, 35, 10, 13)
    Phi, X, G, _, _ = _case(shape, dt)
    Pd, Xd, Gd = Phi.cuda(), X.cuda(), G.cuda()
    full = h.env_half_apply(Pd, Xd, Gd)
    r0, r1, i0, i1, c0, c1, s0, s1 = 5, 30, 3, 9, 2, 12, 7, 33
    part = h.env_half_apply(Pd[r0:r1].contiguous(), Xd[:, :, s0:s1], Gd[:, i0:i1, :, c0:c1])
    assert torch.equal(part, full[r0:r1, i0:i1, c0:c1, s0:s1])
    one = h.env_half_apply(Pd[32:33].contiguous(), Xd[:, :, 34:35], Gd[:, 9:10, :, 12:13])
    assert torch.equal(one, full[32:33, 9:10, 12:13, 34:35])


@pytest.mark.parametrize("dt", DTYPES)
def test_refusals_leave_the_output_untouched(dt):
    L = h.lib()
    shape = (5, 2, 7, 3, 6, 3, 2)
    Phi, X, G, ref, _ = _case(shape, dt)
    Pd, Xd, Gd = Phi.cuda(), X.cuda(), G.cuda()
    out = torch.full((ref.numel(),), SENTINEL, dtype=dt, device="cuda")
    call = functools.partial(_raw, L, dt, Pd, Xd, Gd, out.data_ptr())
    bad_x, bad_g = list(Xd.stride()), list(Gd.stride())
    bad_x[1], bad_g[2] = -bad_x[1], -bad_g[2]
    refused = [
        (call(dtype=7), h.E_INVALID), (call(R=0), h.E_INVALID), (call(A=0), h.E_INVALID), (call(Rp=0), h.E_INVALID),
        (call(J=-1), h.E_INVALID), (call(Sp=0), h.E_INVALID), (call(I=0), h.E_INVALID), (call(Ap=0), h.E_INVALID),
        (call(Phi=None), h.E_INVALID), (call(X=None), h.E_INVALID), (call(G=None), h.E_INVALID), (call(xs=None), h.E_INVALID),
        (call(gs=None), h.E_INVALID), (call(H=None), h.E_INVALID),
        (call(H=Pd.data_ptr()), h.E_INVALID), (call(H=Xd.data_ptr()), h.E_INVALID), (call(H=Gd.data_ptr()), h.E_INVALID),
        (call(xs=_i64(bad_x)), h.E_UNSUPPORTED), (call(gs=_i64(bad_g)), h.E_UNSUPPORTED),
        (call(J=1 << 31), h.E_UNSUPPORTED), (call(A=1 << 16, J=1 << 16), h.E_UNSUPPORTED), (call(I=1 << 20, Ap=1 << 11), h.E_UNSUPPORTED),
        (call(R=1 << 20, A=1 << 20, Rp=1 << 20), h.E_UNSUPPORTED), (call(xs=_i64([1 << 56, 1, 1])), h.E_UNSUPPORTED),
    ]
    for k, (got, want) in enumerate(refused):
        assert got == want, (k, got, want)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert torch.equal(Pd.cpu(), Phi) and torch.equal(Xd.cpu(), X) and torch.equal(Gd.cpu(), G)
    with pytest.raises(ValueError):
        h.env_half_apply(Pd, Xd[:3], Gd)
    with pytest.raises(ValueError):
        h.env_half_apply(Pd, Xd, Gd.to(torch.float64 if dt == torch.float32 else torch.float32))
    with pytest.raises(ValueError, match="Phi must be contiguous"):
        h.env_half_apply(Pd.permute(2, 1, 0).contiguous().permute(2, 1, 0), Xd, Gd)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", [(5, 2, 7, 3, 6, 3, 2), (17, 2, 2, 2, 15, 2, 3), (16, 3, 16, 8, 16, 8, 3)])
def test_unfused_route_agrees(shape, dt):
    """The route on the library's older kernels (ttr_gemm, copy, ttr_ttm_step, copy), which the bench tool times the fused kernel
    against, computes the same H to the same bound."""
    Phi, X, G = sc.operands(shape, dt)
    ref, bound = sc.half_truth_and_bound(Phi, X, G, dt)
    sc.assert_within(_hipops.env_half_apply_unfused(Phi.cuda(), X.cuda(), G.cuda()), ref, bound, "unfused {} {}".format(shape, dt))


# ------------------------------------------------------------------ ops
def _site(dt, R=5, A=3, I=6, S=7, seed=9, symmetric=False):
    g = torch.Generator().manual_seed(seed)
    draw = lambda *s: torch.randn(s, dtype=torch.float64, generator=g).to(dt)  # noqa: E731
    Phi, Psi, G, v = draw(R, A, R), draw(S, A, S), draw(A, I, I, A), draw(R, I, S)
    if symmetric:
        Phi, G = ((Phi + Phi.permute(2, 1, 0)) / 2).to(dt), ((G + G.permute(0, 2, 1, 3)) / 2).to(dt)
    return Phi, G, Psi, v


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("sizes", [(5, 3, 6, 7), (1, 1, 5, 4), (4, 2, 3, 1), (17, 3, 9, 18)])
def test_local_matvec(sizes, dt):
    """B_k v against the dense fp64 contraction, within the chained bound (the kernel's two chains and the GEMM over (a', s'))."""
    R, A, I, S = sizes
    Phi, G, Psi, v = _site(dt, R, A, I, S)
    ref, bound = sc.matvec_truth_and_bound(Phi, G, Psi, v, dt)
    y = _hipops.local_matvec(Phi.cuda(), G.cuda(), Psi.cuda(), v.cuda())
    assert y.is_cuda and y.dtype == dt
    sc.assert_within(y, ref, bound, "local_matvec {} {}".format(sizes, dt))
    Bk = torch.einsum("rab,aijc,tcs->ritbjs", Phi.double(), G.double(), Psi.double()).reshape(R * I * S, R * I * S)
    assert float(((Bk @ v.double().reshape(-1)).reshape(R, I, S) - ref).abs().max()) <= 1e-9 * float(ref.abs().max())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("sizes", [(5, 3, 6, 7), (1, 1, 5, 4), (4, 2, 3, 1), (17, 3, 9, 18)])
def test_env_update(sizes, side, dt):
    R, A, I, S = sizes
    Phi, G, Psi, v = _site(dt, R, A, I, S)
    g = torch.Generator().manual_seed(4)
    bra = torch.randn((R, I, S), dtype=torch.float64, generator=g).to(dt)
    env = Phi if side == "left" else Psi
    ref, bound = sc.env_truth_and_bound(side, env, G, bra, v, dt)
    out = _hipops.env_update(side, env.cuda(), G.cuda(), bra.cuda(), v.cuda())
    sc.assert_within(out, ref, bound, "env_update {} {} {}".format(side, sizes, dt))
    same = bra.cuda()
    ref2, bound2 = sc.env_truth_and_bound(side, env, G, bra, bra, dt)
    sc.assert_within(_hipops.env_update(side, env.cuda(), G.cuda(), same, same), ref2, bound2, "env_update bra is ket {}".format(side))


@pytest.mark.parametrize("dt", DTYPES)
def test_interface_of_a_symmetric_matrix_is_symmetric(dt):
    """With bra == ket, a symmetric interface and core slices symmetric in (i, j), the next interface is symmetric in its outer
    indices in exact arithmetic: the computed one is, to twice the bound."""
    Phi, G, Psi, v = _site(dt, 6, 2, 5, 9, symmetric=True)
    ref, bound = sc.env_truth_and_bound("left", Phi, G, v, v, dt)
    x = v.cuda()
    out = _hipops.env_update("left", Phi.cuda(), G.cuda(), x, x).cpu().double()
    assert float((ref - ref.permute(2, 1, 0)).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert bool(((out - out.permute(2, 1, 0)).abs() <= bound + bound.permute(2, 1, 0)).all())

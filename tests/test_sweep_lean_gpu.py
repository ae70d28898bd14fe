"""The lean builds of ttr_rowgram and ttr_project for `rows32` items (TTR_KNOB_SWEEP_LEAN = 1: fp32 launches of >= 256 items of 64 rows
run a 32-row instance over the flagged items and the generic instance over the rest) against the generic kernel alone (0): same
bits, on both sides of the dispatch threshold, for every mix of flagged and unflagged items in one batch.  Rows 32.. of a flagged
item are NaN here: the contract says they are never loaded, and a build that reads them shows at once."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

T = 256                    # kLeanMinItems of ttr_sweep.hip: launches of fewer items run the generic instance alone
BMAX, NMAX = T + 1, 2048   # at 256 items and 2048 columns the launch has 8 split-K parts (split partials, only split 0 writes `left`)
FLAGS = ("none", "all", "alternating", "last")


def _hip():
    from tntorch_amd import _hip

    _hip.lib()
    return _hip


@functools.lru_cache(maxsize=None)
def _base(dt):
    """Shared inputs on the device: M [BMAX, 64, NMAX + 8] (the cases are views of it), orthogonal V1, V2 [BMAX, 64, 64] (eight
    different matrices each, repeated), sigma [BMAX, 64] in [0.5, 1.5)."""
    g = torch.Generator(device="cuda").manual_seed(1234)
    M = torch.randn(BMAX, 64, NMAX + 8, generator=g, device="cuda", dtype=dt)
    gc = torch.Generator().manual_seed(99)
    Q = torch.linalg.qr(torch.randn(16, 64, 64, generator=gc, dtype=torch.float64))[0].to(dt).cuda()
    idx = torch.arange(BMAX, device="cuda") % 8
    V1, V2 = Q[idx].contiguous(), Q[8 + idx].contiguous()
    sig = (torch.rand(BMAX, 64, generator=gc, dtype=torch.float64) + 0.5).to(dt).cuda()
    return M, V1, V2, sig


def _flags(kind, B):
    f = torch.zeros(B, dtype=torch.int32)
    if kind == "all":
        f[:] = 1
    elif kind == "alternating":
        f[::2] = 1
    elif kind == "last":
        f[-1] = 1
    return f.cuda()


@functools.lru_cache(maxsize=2)
def _inputs(dt, kind, B):
    """(M [B, 64, NMAX + 8] with NaN rows 32.. in the flagged items, flags) -- read-only."""
    f = _flags(kind, B)
    M = _base(dt)[0][:B].clone()
    M[f.bool(), 32:] = float("nan")
    return M, f


def _both(h, fn):
    """fn() with the lean builds off and on."""
    out = {}
    try:
        for v in (0, 1):
            h.set_knob(h.KNOB_SWEEP_LEAN, v)
            out[v] = fn()
    finally:
        h.set_knob(h.KNOB_SWEEP_LEAN, 1)
    return out[0], out[1]


def _project(h, M, V1, V2, sig, ro, scale_right, rows32, pad=0):
    """ttr_project into a right buffer [B, ro, n + pad] preset to -7 (pad > 0: a strided destination) -> (buffer, left)."""
    B, R, n = M.shape
    M, ldm, sM = h._mat(M)
    buf = torch.full((B, ro, n + pad), -7.0, dtype=M.dtype, device=M.device)
    left = torch.full((B, R, ro), -7.0, dtype=M.dtype, device=M.device)
    h._call("ttr_project", h.dtype_code(M.dtype), R, n, ro, B, M.data_ptr(), ldm, sM, h._ptr(V1), 64, 64 * 64, V2.data_ptr(), 64, 64 * 64,
            h._ptr(sig), 64, int(scale_right), buf.data_ptr(), n + pad, ro * (n + pad), left.data_ptr(), ro, R * ro, h._ptr(rows32))
    return buf, left


@pytest.mark.parametrize("kind", FLAGS)
@pytest.mark.parametrize("B", [T - 1, T, T + 1])
def test_lean_rowgram_gives_the_bits_of_the_generic_kernel(B, kind):
    h = _hip()
    M, f = _inputs(torch.float32, kind, B)
    # columns against the ring's prologue and guarded tail: 16 (waves 1 - 3 have no step), 48, 80 (wave 0: two steps), 208, 2048 (8 parts
    # at B >= 256: four steps per wave -- the steady state of the ring starts at seven, see the test below); off = 2: a view that is not
    # 16-byte aligned (element-wise loads)
    for n, off in ((16, 0), (48, 0), (80, 0), (208, 0), (2048, 0), (208, 2)):
        view = M[:, :, off:off + n]
        g0, g1 = _both(h, lambda: h.rowgram(view, rows32=f))
        assert torch.equal(g0, g1), (n, off)
        assert not torch.isnan(g1).any(), (n, off)
        if kind == "all":   # the whole 64 x 64 partial is written: zeros around the 32 x 32 block
            assert not g1[:, :, 32:, :].any() and not g1[:, :, :, 32:].any()


@functools.lru_cache(maxsize=None)
def _long_rows():
    """(M [T, 64, 6680] fp32 with NaN rows 32.. in the flagged items, flags: every other item and the last one)."""
    g = torch.Generator(device="cuda").manual_seed(4321)
    M = torch.randn(T, 64, 6680, generator=g, device="cuda")
    f = _flags("alternating", T)
    f[-1] = 1
    M[f.bool(), 32:] = float("nan")
    return M, f


# The steady state of the slab ring (rowgram_rows32_kernel: NS = 4 steps per round while a wave has >= NS + kLeanAhead = 7 steps left to
# request for).  T items give 8 parts, so a wave has (n / 16 / 8) / 4 steps:
#   n = 4096, aligned:       32 chunks per part, 8 steps per wave: one round, a tail of 4; every part takes the unconditional loads
#   n = 6664, aligned:       417 chunks, the last one ragged (8 columns): parts of 53 chunks -> 14 / 13 / 13 / 13 steps (two rounds, a
#                            tail of 6 / 5), the last part 46 chunks -> 12 / 12 / 11 / 11 steps (tail 4 / 3) with the GUARDED loads
#                            in the ring, the share ending outside n
#   n = 5000, off = 2:       a view that is not 16-byte aligned: guarded element-wise loads in the ring in every part, 40 chunks per
#                            part -> 10 steps (one round, a tail of 6), the last part 33 -> 9 / 8 / 8 / 8
@pytest.mark.parametrize("n,off", [(4096, 0), (6664, 0), (5000, 2)])
def test_lean_rowgram_ring_gives_the_bits_of_the_generic_kernel(n, off):
    h = _hip()
    M, f = _long_rows()
    view = M[:, :, off:off + n]
    assert h.lib().ttr_sweep_gram_parts(n, T) == 8
    g0, g1 = _both(h, lambda: h.rowgram(view, rows32=f))
    assert torch.equal(g0, g1)
    assert not torch.isnan(g1).any()
    Md = torch.nan_to_num(view, nan=0.0).double()   # and the sums are the right ones (bounds: see the last test)
    Gr = Md @ Md.transpose(1, 2)
    assert (g1.double().sum(dim=1) - Gr).abs().max() / Gr.abs().max() < 2e-5


def _launches(fn):
    """Names of the kernels fn() launches."""
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if "ttr" in e.name]


def test_the_lean_instances_are_launched_where_the_dispatch_says():
    """Knob 0 against knob 1 proves nothing if the lean kernels never run: count the launches (lean, generic) of one call."""
    h = _hip()
    _, V1, V2, sig = _base(torch.float32)

    def count(names, lean, generic):
        return sum(lean in x for x in names), sum(generic in x and lean not in x for x in names)

    # (dtype, items, knob, kept rank) -> (lean, generic) launches of rowgram and of project
    cases = (((torch.float32, T, 1, 32), (1, 1), (1, 1)), ((torch.float32, T + 1, 1, 5), (1, 1), (1, 1)),
             ((torch.float32, T, 1, 33), (1, 1), (0, 1)),       # kept rank 33: the projection's generic launch alone
             ((torch.float32, T - 1, 1, 32), (0, 1), (0, 1)),   # below the threshold
             ((torch.float32, T, 0, 32), (0, 1), (0, 1)), ((torch.float64, T, 1, 32), (0, 1), (0, 1)))
    for (dt, B, knob, ro), want_gram, want_proj in cases:
        M, f = _inputs(dt, "alternating", B)
        v1, v2, sg = (x[:B].to(dt) for x in (V1, V2, sig))
        try:
            h.set_knob(h.KNOB_SWEEP_LEAN, knob)
            gram = _launches(lambda: h.rowgram(M[:, :, :208], rows32=f))
            proj = _launches(lambda: _project(h, M[:, :, :208], v1, v2, sg, ro, True, f))
        finally:
            h.set_knob(h.KNOB_SWEEP_LEAN, 1)
        assert count(gram, "rowgram_rows32_kernel", "rotgram_kernel") == want_gram, (dt, B, knob, ro, gram)
        assert count(proj, "project_rows32_kernel", "project_kernel") == want_proj, (dt, B, knob, ro, proj)


@pytest.mark.parametrize("kind", FLAGS)
@pytest.mark.parametrize("B", [T - 1, T, T + 1])
def test_lean_project_gives_the_bits_of_the_generic_kernel(B, kind):
    h = _hip()
    M, f = _inputs(torch.float32, kind, B)
    _, V1, V2, sig = _base(torch.float32)
    V1, V2, sig = V1[:B], V2[:B], sig[:B].clone()
    sig[:, 1] = 1e-40   # below the smallest normal: 1 / sigma counts as 0
    # n = 41: the last pair of columns holds one (element-wise loads and stores in that step)
    for n in (32, 40, 41, 2048):
        for ro in (5, 16, 32, 33):   # 33: the generic launch alone
            for v1 in (V1, None):
                for scale in (True, False):
                    # strided destinations: an even leading dimension (8-byte stores stay) and an odd one (no wide access in the whole
                    # kernel); off = 1: rows of M that are not 8-byte aligned (the same)
                    pad = {(40, 16): 6, (40, 5): 7}.get((n, ro), 0)
                    off = 1 if (n == 41 and ro == 32) else 0
                    (r0, l0), (r1, l1) = _both(h, lambda: _project(h, M[:, :, off:off + n], v1, V2, sig, ro, scale, f, pad))
                    case = (n, ro, v1 is not None, scale)
                    assert torch.equal(r0, r1), case
                    assert torch.equal(l0, l1), case
                    assert not torch.isnan(r1).any() and not torch.isnan(l1).any(), case
                    assert bool((r1[:, :, n:] == -7).all()), case
                    if scale:
                        assert not r1[:, 1, :n].any(), case


@pytest.mark.parametrize("kind", FLAGS)
def test_fp64_never_takes_the_lean_builds(kind):
    h = _hip()
    B = T + 1
    M, f = _inputs(torch.float64, kind, B)
    _, V1, V2, sig = _base(torch.float64)
    for n in (80, 208):
        g0, g1 = _both(h, lambda: h.rowgram(M[:, :, :n], rows32=f))
        assert torch.equal(g0, g1) and not torch.isnan(g1).any()
        (r0, l0), (r1, l1) = _both(h, lambda: _project(h, M[:, :, :n], V1[:B], V2[:B], sig[:B], 32, True, f))
        assert torch.equal(r0, r1) and torch.equal(l0, l1) and not torch.isnan(r1).any()


def test_lean_builds_against_float64():
    """Flagged items against float64 torch with the NaN rows as the zeros they stand for; the bounds of
    tests/test_gpu_kernels.py::test_sweep_gram_rotgram_project."""
    h = _hip()
    B, n, ro, t = T, 208, 32, 2e-5
    M, f = _inputs(torch.float32, "all", B)
    _, V1, V2, sig = _base(torch.float32)
    V1, V2, sig = V1[:B], V2[:B], sig[:B]
    Md = torch.nan_to_num(M[:, :, :n], nan=0.0).double()
    G = h.rowgram(M[:, :, :n], rows32=f).double().sum(dim=1)
    Gr = Md @ Md.transpose(1, 2)
    assert (G - Gr).abs().max() / Gr.abs().max() < t
    assert (G - G.transpose(1, 2)).abs().max() == 0
    U = V1.double() @ V2.double()[:, :, :ro]
    right, left = h.project(M[:, :, :n], V1, V2, sig, ro, scale_right=True, rows32=f)
    assert (right.double() - (U.transpose(1, 2) @ Md) / sig.double()[:, :ro, None]).abs().max() / Md.abs().max() < 4 * t
    assert (left.double() - U * sig.double()[:, None, :ro]).abs().max() < t
    right, left = h.project(M[:, :, :n], None, V2, sig, ro, scale_right=False, rows32=f)
    assert (right.double() - V2.double()[:, :, :ro].transpose(1, 2) @ Md).abs().max() / Md.abs().max() < 4 * t
    assert (left.double() - V2.double()[:, :, :ro]).abs().max() < t

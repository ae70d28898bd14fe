"""ttr_gemm / ttr_gemm_axpby through the raw C ABI on a real MI355X: every kernel of ttr_gemm.hip (three small tiles, split-K and
its reduce kernel, the fp32 128 x 128 kernel with both workgroup maps, the symmetric path) at its tile, split and stride edges.

Method (gemm_cases.py): the operands are views inside NaN-filled buffers with padded leading dimensions and batch strides (a read
past M, N or K returns NaN); the output lies in a buffer filled with a finite sentinel with ldc = N + 5, strideC = M ldc + 7 and
64 guard elements on either side, and everything outside the B M N output elements must keep the sentinel's bits.  Random data is
held to the derived per-element bound 2 (K + 4) u (...), integer data to the exact result, and a second call must repeat the
first bit for bit.  The split-K workspace is handed over filled with NaN: a partial that is read without having been written shows.
Each test prints its largest err / bound ratio (`pytest -s`).
"""
import pytest
import torch

import gemm_cases as gc
from gemm_cases import ALPHA, BETA, SCALE_DIV, SCALE_MUL, SCALE_NONE, Case, Padded, case_id

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
SMALL_PAD, BIG_PAD = (3, 5), (4, 8)   # (ld extra, batch stride extra) of the inputs; the big kernel needs multiples of 4
PLAIN = {}
SCALES = {"rs_mode": SCALE_DIV, "cs_mode": SCALE_MUL}
AXPBY = {"alpha": ALPHA, "beta": BETA}
VARIANTS = {"plain": PLAIN, "scales": SCALES, "axpby": AXPBY}


def _hip():
    from tntorch_amd import _hip

    _hip.lib()
    return _hip


@pytest.fixture
def big_knob():
    """TTR_KNOB_GEMM_BIG for the test to turn; put back to its default afterwards."""
    h = _hip()
    try:
        yield lambda v: h.set_knob(h.KNOB_GEMM_BIG, v)
    finally:
        h.set_knob(h.KNOB_GEMM_BIG, 1)


def workspace_bytes(case, dt):
    h = _hip()
    return h.lib().ttr_gemm_workspace_bytes(h.dtype_code(dt), case.M, case.N, case.K, case.B)


def run(case, dt, ops, rs_mode=SCALE_NONE, cs_mode=SCALE_NONE, alpha=None, beta=None, ws="full", pad=SMALL_PAD, a_ld_extra=None,
        a_offset=0, broadcast_b=False, same=False, c_nan=False, what=""):
    """One product through the raw ABI, twice (equal bits), guards checked: the [B, M, N] result on the CPU."""
    h = _hip()
    L = h.lib()
    M, N, K, tA, tB, B = case
    a = Padded.of(ops.A, pad[0] if a_ld_extra is None else a_ld_extra, pad[1], NAN, DEV, a_offset)
    b = a if same else Padded.of(ops.Bm, pad[0], pad[1], NAN, DEV)
    stride_b = 0 if broadcast_b else b.stride
    assert not broadcast_b or ops.Bm.shape[0] == 1
    rs = Padded.of(ops.rs[:, None, :], 3, 0, NAN, DEV) if rs_mode != SCALE_NONE else None
    cs = Padded.of(ops.cs[:, None, :], 3, 0, NAN, DEV) if cs_mode != SCALE_NONE else None
    c = Padded((B, M, N), dt, N + 5, M * (N + 5) + 7, gc.SENTINEL, DEV)
    wsb = L.ttr_gemm_workspace_bytes(h.dtype_code(dt), M, N, K, B)
    wbuf = torch.full((max(wsb, 1),), 0xFF, dtype=torch.uint8, device=DEV)   # (all ones: NaN in fp32 and in fp64)
    ws_ptr, ws_bytes = {"full": (wbuf.data_ptr(), wsb), "null": (None, 0), "short": (wbuf.data_ptr(), wsb - 1)}[ws]
    c0 = None if alpha is None else (torch.full((B, M, N), NAN, dtype=dt) if c_nan else ops.C).to(DEV)
    outs = []
    for _ in range(2):
        c.refill(c0)
        wbuf.fill_(0xFF)
        if alpha is None:
            rc = L.ttr_gemm(h.dtype_code(dt), int(tA), int(tB), M, N, K, a.ptr(), a.ld, a.stride, b.ptr(), b.ld, stride_b,
                            c.ptr(), c.ld, c.stride, rs.ptr() if rs else None, rs.stride if rs else 0, rs_mode,
                            cs.ptr() if cs else None, cs.stride if cs else 0, cs_mode, B, ws_ptr, ws_bytes, h._stream())
        else:
            rc = L.ttr_gemm_axpby(h.dtype_code(dt), int(tA), int(tB), M, N, K, a.ptr(), a.ld, a.stride, b.ptr(), b.ld, stride_b,
                                  c.ptr(), c.ld, c.stride, float(alpha), float(beta), B, ws_ptr, ws_bytes, h._stream())
        assert rc == 0, (what, rc, L.ttr_last_error())
        torch.cuda.synchronize()
        buf = c.buf.cpu()
        gc.assert_guards(c, buf, what)
        outs.append(c.view(buf).clone())
    bits = torch.int32 if dt == torch.float32 else torch.int64
    assert torch.equal(outs[0].view(bits), outs[1].view(bits)), f"{what}: a second call gives other bits"
    return outs[0]


def within(group, got, truth, bound, what):
    """assert_within, with the largest err / bound printed first."""
    r, idx = gc.worst_ratio(got, truth, bound)
    print(f"ratio[{group}] {r:.3e} at {idx}: {what}")
    gc.assert_within(got, truth, bound, what)


def check(group, case, dt, variant=PLAIN, **kw):
    """The case on integer data (exact) and on random data (bound)."""
    what = f"{group} {case_id(case)} {str(dt)[6:]} {variant} {kw}"
    for draw, exact in ((gc.int_operands, True), (gc.operands, False)):
        ops = draw(case, dt)
        if kw.get("broadcast_b"):
            ops = ops._replace(Bm=ops.Bm[:1].contiguous())   # (the fp64 truth broadcasts it as the kernel does)
        truth, bound = gc.truth_and_bound(case, ops, dt, **variant)
        got = run(case, dt, ops, what=what, **variant, **kw)
        if exact:
            gc.assert_exact(got, truth, what + " (integers)")
        else:
            within(group, got, truth, bound, what)


# ------------------------------------------------------------------ 1. small-tile kernels
@pytest.mark.parametrize("dt", gc.DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", gc.SMALL_CASES, ids=case_id)
def test_small_tiles(case, dt):
    assert workspace_bytes(case, dt) == 0
    check("small", case, dt)


@pytest.mark.parametrize("dt", gc.DTYPES, ids=["f32", "f64"])
def test_small_tiles_broadcast_operand(dt):
    """strideB = 0: the three items share one B."""
    check("small", gc.BROADCAST_CASE, dt, broadcast_b=True)


# ------------------------------------------------------------------ 2. small-path split-K
@pytest.mark.parametrize("dt", gc.DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case", gc.SPLIT_CASES, ids=case_id)
def test_small_split_k(case, variant, dt):
    """Few tiles and K >= 2048: partial products per K range, then the reduce kernel, which also applies the scales / the axpby."""
    assert workspace_bytes(case, dt) > 0
    check("split", case, dt, VARIANTS[variant])


@pytest.mark.parametrize("dt", gc.DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("ws", ["null", "short"])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case", gc.SPLIT_CASES, ids=case_id)
def test_split_shape_without_a_sufficient_workspace_runs_unsplit(case, variant, ws, dt):
    """workspace = NULL, or one byte short of ttr_gemm_workspace_bytes: status 0 and the same bound (one split, no partials)."""
    assert workspace_bytes(case, dt) > 0
    check("split-no-ws", case, dt, VARIANTS[variant], ws=ws)


# ------------------------------------------------------------------ 3. big-tile kernel
@pytest.mark.parametrize("case", gc.BIG_CASES + [gc.BIG_NINE_ROW_TILES], ids=case_id)
def test_big_tiles(case, big_knob):
    """fp32, M, N >= 128, K >= 64, multiples of 4, aligned: the 128 x 128 kernel (knob 1) and the 64 x 64 kernel (knob 0) both give
    the exact integers and stay within the bound."""
    dt = torch.float32
    for knob in (1, 0):
        big_knob(knob)
        check(f"big-knob{knob}", case, dt, pad=BIG_PAD)


@pytest.mark.parametrize("edge", list(gc.BIG_FALLBACKS))
def test_big_tile_eligibility_edges_fall_back(edge, big_knob):
    """One step outside the big kernel's envelope (an extent that is no multiple of 4 or below the minimum, a leading dimension
    that is no multiple of 4, a base pointer that is not 16-byte aligned): the 64 x 64 kernel runs, same checks."""
    case, ld_extra, off = gc.BIG_FALLBACKS[edge]
    check("big-fallback", case, torch.float32, pad=BIG_PAD, a_ld_extra=ld_extra, a_offset=off)


@pytest.mark.parametrize("variant", ["scales", "axpby"])
def test_big_tile_epilogue(variant, big_knob):
    for knob in (1, 0):
        big_knob(knob)
        check(f"big-knob{knob}", gc.BIG_RAGGED, torch.float32, VARIANTS[variant], pad=BIG_PAD)


# ------------------------------------------------------------------ 4. big split-K
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_big_split_k(variant):
    """Four tiles and K = 16384: K splits on the 8-way map, partial tiles, the reduce kernel (with the axpby / the scales)."""
    assert workspace_bytes(gc.BIG_SPLIT_CASE, torch.float32) > 0
    check("big-split", gc.BIG_SPLIT_CASE, torch.float32, VARIANTS[variant], pad=BIG_PAD)


def test_big_split_shape_without_a_workspace_runs_unsplit():
    """(ttr_gemm_workspace_bytes covers the deepest split of any path for the shape, so "one byte short" of it says nothing
    about this path: NULL only.)"""
    check("big-split-no-ws", gc.BIG_SPLIT_CASE, torch.float32, AXPBY, pad=BIG_PAD, ws="null")


# ------------------------------------------------------------------ 5. symmetric products
def _census_flops(fn):
    h = _hip()
    h.prof_enable(2)
    try:
        out = fn()
        torch.cuda.synchronize()
        h.prof_collect()
        work = h.prof_collect_work()
    finally:
        h.prof_enable(False)
    return out, work["gemm"]["flops"]


@pytest.mark.parametrize("side,rows,cols", gc.SYM_CASES, ids=[f"{s}-{r}x{c}" for s, r, c in gc.SYM_CASES])
def test_symmetric_products(side, rows, cols):
    """The same pointer on both sides, transposed on one: only the tiles on and above the diagonal run and are mirrored on output
    (through the partials at the split shape) -- the ragged edge tiles (132, 260) included."""
    dt = torch.float32
    case = gc.sym_case(side, rows, cols, B=2 if rows < 1000 else 1)
    M, K = case.M, case.K
    if rows >= 1000:
        assert workspace_bytes(case, dt) > 0
    what = f"sym {side} {rows}x{cols}"
    g = torch.Generator().manual_seed(rows + cols)
    Ai = torch.randint(-3, 4, (case.B, rows, cols), generator=g).to(dt)
    Ar = torch.randn((case.B, rows, cols), generator=g, dtype=torch.float64).to(dt)
    for A, exact in ((Ai, True), (Ar, False)):
        ops = gc.Ops(A, A, None, None, None)
        truth, bound = gc.truth_and_bound(case, ops, dt)
        got, flops = _census_flops(lambda: run(case, dt, ops, pad=BIG_PAD, same=True, what=what))
        assert torch.equal(got, got.transpose(1, 2)), f"{what}: C != C^T"
        # the census counts what the path computes: the upper tile triangle (run() calls twice)
        assert flops == pytest.approx(2 * case.B * 2.0 * M * M * K * 0.5 * (1 + 128 / M), rel=1e-12), f"{what}: not the triangular path"
        # the same data as a separate copy: the general path, every tile
        sep, flops = _census_flops(lambda: run(case, dt, ops, pad=BIG_PAD, what=what + " (copy)"))
        assert flops == pytest.approx(2 * case.B * 2.0 * M * M * K, rel=1e-12)
        if exact:
            gc.assert_exact(got, truth, what)
            gc.assert_exact(sep, truth, what + " (copy)")
        else:
            within("symmetric", got, truth, bound, what)
            within("symmetric-copy", sep, truth, bound, what + " (copy)")


# ------------------------------------------------------------------ 6. beta = 0 does not read C
BETA0 = {"small": (Case(65, 63, 17, False, False, 2), gc.DTYPES, SMALL_PAD), "split": (gc.SPLIT_CASES[3], gc.DTYPES, SMALL_PAD),
         "big": (gc.BIG_RAGGED, [torch.float32], BIG_PAD), "big-split": (gc.BIG_SPLIT_CASE, [torch.float32], BIG_PAD)}


@pytest.mark.parametrize("kind,dt", [(k, dt) for k, v in BETA0.items() for dt in v[1]],
                         ids=[f"{k}-{str(dt)[6:]}" for k, v in BETA0.items() for dt in v[1]])
def test_axpby_with_beta_zero_does_not_read_c(kind, dt):
    """C <- 0 * C + alpha A B with C full of NaN: finite and within the bound of alpha A B."""
    case, _, pad = BETA0[kind]
    if "split" in kind:
        assert workspace_bytes(case, dt) > 0
    check(f"beta0-{kind}", case, dt, {"alpha": ALPHA, "beta": 0.0}, pad=pad, c_nan=True)


# ------------------------------------------------------------------ 7. TTR_SCALE_DIV around the smallest normal
@pytest.mark.parametrize("dt", gc.DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("path", ["direct", "reduce"])
@pytest.mark.parametrize("side", ["row", "col"])
def test_scale_div_threshold(side, path, dt):
    """x / s is exactly 0 for |s| below the smallest normal (0, -0, both ends of the subnormal range) and the quotient at it."""
    case = Case(65, 63, 17, False, False, 2) if path == "direct" else gc.SPLIT_CASES[5]
    assert (workspace_bytes(case, dt) > 0) == (path == "reduce")
    ops = gc.operands(case, dt)
    thr = gc.threshold_scales(dt)
    s = (ops.rs if side == "row" else ops.cs).clone()
    s[0, 1:7], s[-1, -6:] = thr, thr.flip(0)
    # |A B| << 1 so that the quotient by the smallest normal is finite
    ops = ops._replace(A=ops.A * 2.0 ** -12, **({"rs": s} if side == "row" else {"cs": s}))
    modes = {"rs_mode": SCALE_DIV, "cs_mode": SCALE_MUL} if side == "row" else {"rs_mode": SCALE_MUL, "cs_mode": SCALE_DIV}
    truth, bound = gc.truth_and_bound(case, ops, dt, **modes)
    assert torch.isfinite(truth).all()
    what = f"div-threshold {side} {path} {dt}"
    got = run(case, dt, ops, what=what, **modes)
    dead = (s.abs() < torch.finfo(dt).tiny)
    dead = dead[:, :, None].expand_as(got) if side == "row" else dead[:, None, :].expand_as(got)
    assert dead.sum() == 8 * (case.N if side == "row" else case.M)
    assert (got[dead] == 0).all(), f"{what}: a scale below the smallest normal must give exactly 0"
    assert (got[~dead] != 0).all()
    within("div-threshold", got, truth, bound, what)


# ------------------------------------------------------------------ 8. refusals
def _raw(entry, dtype_code, M, N, K, batch, a, b, c, null=None):
    h = _hip()
    L = h.lib()
    p = {"A": a.ptr(), "B": b.ptr(), "C": c.ptr()}
    if null:
        p[null] = None
    head = (dtype_code, 0, 0, M, N, K, p["A"], a.ld, a.stride, p["B"], b.ld, b.stride, p["C"], c.ld, c.stride)
    if entry == "ttr_gemm":
        return L.ttr_gemm(*head, None, 0, SCALE_NONE, None, 0, SCALE_NONE, batch, None, 0, h._stream())
    return L.ttr_gemm_axpby(*head, ALPHA, BETA, batch, None, 0, h._stream())


REFUSED = {"bad dtype": dict(dtype_code=7), "M < 0": dict(M=-1), "N < 0": dict(N=-1), "K < 0": dict(K=-1), "batch < 0": dict(batch=-1),
           "K = 0": dict(K=0), "null A": dict(null="A"), "null B": dict(null="B"), "null C": dict(null="C")}
EMPTY = {"M = 0": dict(M=0), "N = 0": dict(N=0), "batch = 0": dict(batch=0), "M = 0, null C": dict(M=0, null="C")}


@pytest.mark.parametrize("entry", ["ttr_gemm", "ttr_gemm_axpby"])
@pytest.mark.parametrize("dt", gc.DTYPES, ids=["f32", "f64"])
def test_refusals_and_empty_products_leave_the_output_untouched(dt, entry):
    h = _hip()
    M, N, K, B = 5, 7, 3, 2
    ops = gc.operands(Case(M, N, K, False, False, B), dt)
    a, b = Padded.of(ops.A, 3, 5, NAN, DEV), Padded.of(ops.Bm, 3, 5, NAN, DEV)
    c = Padded((B, M, N), dt, N + 5, M * (N + 5) + 7, gc.SENTINEL, DEV)
    base = dict(dtype_code=h.dtype_code(dt), M=M, N=N, K=K, batch=B)
    for table, ok in ((REFUSED, False), (EMPTY, True)):
        for name, change in table.items():
            rc = _raw(entry, a=a, b=b, c=c, **{**base, **change})
            torch.cuda.synchronize()
            assert (rc == 0) == ok, (name, rc)
            if not ok:
                assert rc == h.E_INVALID and h.lib().ttr_last_error(), name
            gc.assert_guards(c, c.buf.cpu(), f"{entry} {name}", window=False)
    assert _raw(entry, a=a, b=b, c=c, **base) == 0               # the unchanged call is accepted and writes
    torch.cuda.synchronize()
    assert torch.isfinite(c.view()).all() and (c.view() != gc.SENTINEL).all()
    gc.assert_guards(c, c.buf.cpu(), entry)

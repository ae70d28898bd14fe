"""The sweep kernels (ttr_sweep.hip) through the raw C ABI on a real MI355X, entry-wise against fp64 truths: ttr_rowgram,
ttr_rotgram, ttr_project / ttr_project_flat, ttr_colgram, ttr_colproject on graded data and at their tile, tail, split, layout,
flag, knob and grid-limit edges, and ttr_spectrum_flat / ttr_carry_rows32 at their thresholds.

Method (sweep_cases.py, whose docstring derives every bound): inputs are views inside NaN-filled buffers (a read outside the
contract returns NaN: the padding columns, rows 32.. of a `rows32` item, V2 and sigma of a pass-through item, the colgram
workspace), outputs lie inside sentinel-filled buffers with guards that must keep their bits.  Every result is held to its own
entry-wise bound: an entry of the rotated Gram matrix that belongs to two small rows has a bound of its own size, which a
one-pass V1^T (M M^T) V1 misses by two orders of magnitude (test_sweep_cases_host.py) while a norm-wise comparison passes it.
Flags are checked against the truth, not against another knob value.  Each test prints its largest error / bound (`pytest -s`).
"""
import functools

import pytest
import torch

import sweep_cases as sc
from gemm_cases import SENTINEL, Padded, assert_guards
from matrix_cases import assert_within

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
DT = pytest.mark.parametrize("dt", sc.DTYPES, ids=["f32", "f64"])
LEAN_B = 256    # kLeanMinItems of ttr_sweep.hip: fp32 launches of >= 256 items of 64 rows run the lean instances over the flagged items


def _hip():
    from tntorch_amd import _hip

    _hip.lib()
    return _hip


def raw(name, *args):
    """The entry point's return code (the stream is appended), after the device has finished."""
    h = _hip()
    rc = getattr(h.lib(), name)(*args, h._stream())
    torch.cuda.synchronize()
    return rc


def call(name, *args):
    rc = raw(name, *args)
    assert rc == 0, (name, rc, _hip().lib().ttr_last_error())


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def ptr(t):
    return None if t is None else t.data_ptr()


def flags(values):
    return None if values is None else torch.as_tensor(values, dtype=torch.int32).to(DEV)


def nan_bytes(nbytes):
    """A device buffer of all-ones bytes: NaN in fp32 and in fp64."""
    return torch.full((max(int(nbytes), 1),), 0xFF, dtype=torch.uint8, device=DEV)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def is_sentinel(t):
    return same_bits(t, torch.full_like(t, SENTINEL))


def fetch(p, what):
    """The window of an output after a kernel ran; everything around it must have kept the fill's bits."""
    buf = p.buf.cpu()
    assert_guards(p, buf, what)
    return p.view(buf).clone()


class knob:
    """`with knob(h.KNOB_X, v):` -- set, and restored to the library's default afterwards."""

    def __init__(self, which, value, default=1):
        self.which, self.value, self.default = which, value, default

    def __enter__(self):
        _hip().set_knob(self.which, self.value)

    def __exit__(self, *exc):
        _hip().set_knob(self.which, self.default)


# ------------------------------------------------------------------ runners: one raw call each, guarded outputs
def run_gram(dt, M, V1=None, nparts=None, skip=None, rows32=None, layout=(0, 0), what="gram"):
    """ttr_rowgram (V1 None) / ttr_rotgram -> the parts [B, nparts, R, R].  layout = (ldm - n, elements the base lies off its
    16-byte boundary); M sits in a NaN-filled buffer."""
    h = _hip()
    B, R, n = M.shape
    if nparts is None:
        nparts = int(h.lib().ttr_sweep_gram_parts(n, B))
    m = Padded.of(M, layout[0], 0, NAN, DEV, layout[1])
    g = Padded((1, B * nparts * R, R), dt, R, 0, SENTINEL, DEV)
    code = h.dtype_code(dt)
    f32, fsk = flags(rows32), flags(skip)
    if V1 is None:
        assert skip is None
        call("ttr_rowgram", code, R, n, B, m.ptr(), m.ld, m.stride, g.ptr(), nparts, ptr(f32))
    else:
        v = dev(V1)
        call("ttr_rotgram", code, R, n, B, m.ptr(), m.ld, m.stride, v.data_ptr(), R, R * R, g.ptr(), nparts, ptr(fsk), ptr(f32))
    return fetch(g, what).reshape(B, nparts, R, R)


def run_project(dt, M, V1, V2, sigma, ro, scale, rows32=None, flat=None, sigma1=None, m_layout=(0, 0), r_layout=(0, 0), ldl_extra=0,
                want_left=True, what="project"):
    """ttr_project_flat -> (right [B, ro, n], left [B, R, ro] or None).  r_layout = (ldr - n, base offset) of `right`."""
    h = _hip()
    B, R, n = M.shape
    m = Padded.of(M, m_layout[0], 0, NAN, DEV, m_layout[1])
    ldr, ldl = n + r_layout[0], ro + ldl_extra
    r = Padded((B, ro, n), dt, ldr, ro * ldr, SENTINEL, DEV, r_layout[1])
    l = Padded((B, R, ro), dt, ldl, R * ldl, SENTINEL, DEV)
    v1, v2, sg, s1 = dev(V1), dev(V2), dev(sigma), dev(sigma1)
    f32, ffl = flags(rows32), flags(flat)
    call("ttr_project_flat", h.dtype_code(dt), R, n, ro, B, m.ptr(), m.ld, m.stride, ptr(v1), R, R * R, v2.data_ptr(), R, R * R,
         ptr(sg), sg.shape[-1] if sg is not None else 0, int(scale), r.ptr(), r.ld, r.stride, l.ptr() if want_left else None, l.ld,
         l.stride, ptr(f32), ptr(ffl), ptr(s1), s1.shape[-1] if s1 is not None else 0)
    right = fetch(r, what + " right")
    if not want_left:
        assert_guards(l, l.buf.cpu(), what + " left (not asked for)", window=False)
        return right, None
    return right, fetch(l, what + " left")


def run_colgram(dt, M, V1=None, skip=None, layout=(0, 0), what="colgram"):
    """ttr_colgram of the tall M [B, rows, n] -> G [B, n, n]; the workspace is NaN before the call."""
    h = _hip()
    B, rows, n = M.shape
    code = h.dtype_code(dt)
    m = Padded.of(M, layout[0], 0, NAN, DEV, layout[1])
    g = Padded((B, n, n), dt, n, n * n, SENTINEL, DEV)
    wsb = int(h.lib().ttr_colgram_workspace_bytes(code, rows, n, B))
    parts = sc.col_split(rows, B)
    assert wsb == (parts * B * n * n * (4 if dt == torch.float32 else 8) if parts > 1 else 0)
    ws = nan_bytes(wsb)
    v, fsk = dev(V1), flags(skip)
    call("ttr_colgram", code, rows, n, B, m.ptr(), m.ld, m.stride, ptr(v), n, n * n, g.ptr(), ws.data_ptr() if wsb else None, wsb, ptr(fsk))
    return fetch(g, what)


def run_colproject(dt, M, V1, V2, sigma, ro, left_ortho, layout=(0, 0), l_layout=(0, 0), ldr_extra=0, what="colproject"):
    """ttr_colproject -> (left [B, rows, ro], right [B, ro, n])."""
    h = _hip()
    B, rows, n = M.shape
    m = Padded.of(M, layout[0], 0, NAN, DEV, layout[1])
    ldl, ldr = ro + l_layout[0], n + ldr_extra
    l = Padded((B, rows, ro), dt, ldl, rows * ldl, SENTINEL, DEV, l_layout[1])
    r = Padded((B, ro, n), dt, ldr, ro * ldr, SENTINEL, DEV)
    v1, v2, sg = dev(V1), dev(V2), dev(sigma)
    call("ttr_colproject", h.dtype_code(dt), rows, n, ro, B, m.ptr(), m.ld, m.stride, ptr(v1), n, n * n, v2.data_ptr(), n, n * n, ptr(sg),
         sg.shape[-1] if sg is not None else 0, int(left_ortho), l.ptr(), l.ld, l.stride, r.ptr(), r.ld, r.stride)
    return fetch(l, what + " left"), fetch(r, what + " right")


def check_project(got, truth, what):
    right, rb, left, lb = truth
    assert_within(got[0], right, rb, what + " right")
    if got[1] is not None:
        assert_within(got[1], left, lb, what + " left")


def check_colproject(got, truth, what):
    left, lb, right, rb = truth
    assert_within(got[0], left, lb, what + " left")
    assert_within(got[1], right, rb, what + " right")


def tall(M):
    return M.transpose(1, 2).contiguous()


# ------------------------------------------------------------------ graded data, entry-wise
@DT
@pytest.mark.parametrize("case", sc.GRADED, ids=lambda c: "R{}-n{}-d{}".format(*c))
def test_graded_gram(dt, case):
    """Three graded items scaled by 1, 2^20, 2^-20: the Gram matrix of the rotated rows carries its small entries to THEIR size."""
    R, n, decay = case
    M, V1, _, _, _ = sc.graded_batch(R, n, decay, dt)
    parts = sc.pick_split(n, 3)
    tag = "R={} n={} decay={} {}".format(R, n, decay, sc.dt_name(dt))
    G = run_gram(dt, M).double().sum(dim=1)
    assert_within(G, *sc.gram_truth_and_bound(M, None, dt, parts), "rowgram graded " + tag)
    G2 = run_gram(dt, M, V1)
    assert G2.shape[1] == parts and same_bits(G2, G2.transpose(2, 3))
    assert_within(G2.double().sum(dim=1), *sc.gram_truth_and_bound(M, V1, dt, parts), "rotgram graded " + tag)
    Mt = tall(M)                                          # the tall kernels: n rows, R columns
    cparts = sc.col_split(n, 3)
    assert_within(run_colgram(dt, Mt), *sc.colgram_truth_and_bound(Mt, None, dt, cparts), "colgram graded " + tag)
    assert_within(run_colgram(dt, Mt, V1), *sc.colgram_truth_and_bound(Mt, V1, dt, cparts), "colgram rotated graded " + tag)


@DT
@pytest.mark.parametrize("case", sc.GRADED, ids=lambda c: "R{}-n{}-d{}".format(*c))
def test_graded_project(dt, case):
    """V1 given and U handed over ready, both scalings, `left` with ldl > ro; kept rank R / 2 and R (fp32: the last sigma of pass 2
    are zeros -- their rows of `right` must be exact zeros)."""
    R, n, decay = case
    M, V1, V2, sigma, _ = sc.graded_batch(R, n, decay, dt)
    Uready = (V1.double() @ V2.double()).to(dt)
    Mt = tall(M)
    for ro in (R // 2, R):
        for v1, v2 in ((V1, V2), (None, Uready)):
            for scale in (1, 0):
                tag = "graded R={} n={} ro={} {}{} {}".format(R, n, ro, "V1" if v1 is not None else "noV1", " scaled" if scale else "", sc.dt_name(dt))
                got = run_project(dt, M, v1, v2, sigma, ro, scale, ldl_extra=3, what=tag)
                check_project(got, sc.project_truth_and_bounds(M, v1, v2, sigma, ro, scale, dt), "project " + tag)
                got = run_colproject(dt, Mt, v1, v2, sigma, ro, scale, ldr_extra=3, what=tag)
                check_colproject(got, sc.colproject_truth_and_bounds(Mt, v1, v2, sigma, ro, scale, dt), "colproject " + tag)


# ------------------------------------------------------------------ tile and tail edges (randn, the same bounds)
@DT
@pytest.mark.parametrize("R", sc.GRAM_R)
def test_gram_tile_edges(dt, R):
    """Waves without a step (n <= 48), the ragged last chunk, row tiles that end inside a tile."""
    for n in sc.GRAM_N:
        M, V1, _, _, _ = sc.random_batch(2, R, n, dt)
        tag = "R={} n={} {}".format(R, n, sc.dt_name(dt))
        assert_within(run_gram(dt, M).double().sum(dim=1), *sc.gram_truth_and_bound(M, None, dt, 1), "rowgram edges " + tag)
        assert_within(run_gram(dt, M, V1).double().sum(dim=1), *sc.gram_truth_and_bound(M, V1, dt, 1), "rotgram edges " + tag)


@DT
@pytest.mark.parametrize("n", sc.PROJECT_N)
def test_project_tile_edges(dt, n):
    shapes = [(64, ro) for ro in sc.PROJECT_RO_64] + [(R, ro) for R in sc.PROJECT_SMALL_R for ro in sorted({1, R})]
    for k, (R, ro) in enumerate(shapes):
        M, V1, V2, sigma, _ = sc.random_batch(2, R, n, dt)
        for v1, scale in ((V1, 1), (None, 0)) if k % 2 == 0 else ((V1, 0), (None, 1)):
            tag = "edges R={} ro={} n={} {}{} {}".format(R, ro, n, "V1" if v1 is not None else "noV1", " scaled" if scale else "", sc.dt_name(dt))
            got = run_project(dt, M, v1, V2, sigma, ro, scale, what=tag)
            check_project(got, sc.project_truth_and_bounds(M, v1, V2, sigma, ro, scale, dt), "project " + tag)


@DT
@pytest.mark.parametrize("n,parts", sc.PROJECT_SPLIT_N)
def test_project_split_edges(dt, n, parts):
    """Two items: 2 and 4 column parts, the last share ragged, `left` written by part 0 alone (once: the guards and the values)."""
    h = _hip()
    assert int(h.lib().ttr_sweep_gram_parts(n, 2)) == parts == sc.pick_split(n, 2)
    for R, ro in ((64, 33), (37, 37)):
        M, V1, V2, sigma, _ = sc.random_batch(2, R, n, dt)
        tag = "split R={} ro={} n={} {}".format(R, ro, n, sc.dt_name(dt))
        got = run_project(dt, M, V1, V2, sigma, ro, 1, ldl_extra=1, what=tag)
        check_project(got, sc.project_truth_and_bounds(M, V1, V2, sigma, ro, 1, dt), "project " + tag)
        assert_within(run_gram(dt, M, V1).double().sum(dim=1), *sc.gram_truth_and_bound(M, V1, dt, parts), "rotgram " + tag)


@DT
@pytest.mark.parametrize("n", sc.COL_N)
def test_col_tile_edges(dt, n):
    for k, rows in enumerate(sc.COL_ROWS):
        Mr, V1, V2, sigma, _ = sc.random_batch(2, n, rows, dt)
        M = tall(Mr)
        tag = "rows={} n={} {}".format(rows, n, sc.dt_name(dt))
        assert_within(run_colgram(dt, M), *sc.colgram_truth_and_bound(M, None, dt, 1), "colgram edges " + tag)
        assert_within(run_colgram(dt, M, V1), *sc.colgram_truth_and_bound(M, V1, dt, 1), "colgram rotated edges " + tag)
        for ro in sorted({1, (n + 1) // 2, n}):
            for v1, scale in ((V1, 1), (None, 0)) if k % 2 == 0 else ((V1, 0), (None, 1)):
                t2 = "{} ro={} {}{}".format(tag, ro, "V1" if v1 is not None else "noV1", " scaled" if scale else "")
                got = run_colproject(dt, M, v1, V2, sigma, ro, scale, what=t2)
                check_colproject(got, sc.colproject_truth_and_bounds(M, v1, V2, sigma, ro, scale, dt), "colproject edges " + t2)


@DT
@pytest.mark.parametrize("rows,parts", sc.COL_SPLIT_ROWS)
def test_col_split_edges(dt, rows, parts):
    """Two items: 3 and 4 row parts, the last ragged; the partials are summed from a workspace that was NaN before the call."""
    assert sc.col_split(rows, 2) == parts
    for n in (64, 33):
        Mr, V1, V2, sigma, _ = sc.random_batch(2, n, rows, dt)
        M = tall(Mr)
        tag = "split rows={} n={} {}".format(rows, n, sc.dt_name(dt))
        assert_within(run_colgram(dt, M), *sc.colgram_truth_and_bound(M, None, dt, parts), "colgram " + tag)
        assert_within(run_colgram(dt, M, V1), *sc.colgram_truth_and_bound(M, V1, dt, parts), "colgram rotated " + tag)
        ro = n // 2
        got = run_colproject(dt, M, V1, V2, sigma, ro, 1, ldr_extra=2, what=tag)
        check_colproject(got, sc.colproject_truth_and_bounds(M, V1, V2, sigma, ro, 1, dt), "colproject " + tag)


# ------------------------------------------------------------------ a caller-chosen nparts
@DT
@pytest.mark.parametrize("nparts", sc.NPARTS)
def test_caller_chosen_nparts(dt, nparts):
    """n = 100: 7 chunks of 16 columns in 1, 3, 7 and 9 parts -- uneven shares and parts without a chunk, which are exact zeros."""
    n = sc.NPARTS_N
    for R in (64, 37):
        M, V1, _, _, _ = sc.random_batch(3, R, n, dt)
        for v1 in (None, V1):
            tag = "{} nparts={} R={} {}".format("rotgram" if v1 is not None else "rowgram", nparts, R, sc.dt_name(dt))
            got = run_gram(dt, M, v1, nparts=nparts, what=tag)
            G, bound = sc.part_truths_and_bounds(M, v1, dt, nparts)
            assert_within(got, G, bound, tag + " parts")
            for q in range(nparts):
                if sc.part_columns(n, nparts, q)[0] == n:
                    assert not got[:, q].any(), (tag, q)


@pytest.mark.parametrize("nparts", sc.NPARTS)
def test_caller_chosen_nparts_lean(nparts):
    """The lean instance (fp32, 256 items of 64 rows, every item flagged, rows 32.. NaN): the same parts, zeros around the 32 x 32 block."""
    dt, n, B = torch.float32, sc.NPARTS_N, LEAN_B
    M = sc.random_batch(B, 64, n, dt)[0].clone()
    M[:, 32:] = NAN
    f = [1] * B
    got = run_gram(dt, M, None, nparts=nparts, rows32=f, what="lean rowgram nparts={}".format(nparts))
    G, bound = sc.part_truths_and_bounds(M, None, dt, nparts, rows32=f)
    assert_within(got, G, bound, "lean rowgram nparts={} parts".format(nparts))
    assert not got[:, :, 32:, :].any() and not got[:, :, :, 32:].any()
    for q in range(nparts):
        if sc.part_columns(n, nparts, q)[0] == n:
            assert not got[:, q].any(), q


# ------------------------------------------------------------------ layout: leading dimensions and base alignment
def _odd(n):
    return 1 if n % 2 == 0 else 2


@DT
def test_layouts_give_the_bits_of_the_contiguous_call(dt):
    """ldm > n, odd ldm / ldr, bases one, two and three elements off a 16-byte boundary: the element-wise paths compute the
    same sums.  The padding columns keep their fill (the runners' guards)."""
    for R, n, B in ((64, 100, 2), (37, 65, 2), (64, 208, LEAN_B)):
        if B == LEAN_B and dt != torch.float32:
            continue
        M, V1, V2, sigma, _ = sc.random_batch(B, R, n, dt)
        f = None
        if B == LEAN_B:      # the lean instances: every other item flagged
            f = [b % 2 for b in range(B)]
            M = M.clone()
            M[torch.tensor(f).bool(), 32:] = NAN
        ro = R // 2
        layouts = ((4, 0), (_odd(n), 0), (0, 1), (_odd(n), 2), (4, 3), (_odd(n) + 2, 1))
        ref_row = run_gram(dt, M, rows32=f)
        ref_rot = run_gram(dt, M, V1, rows32=f)
        ref_r, ref_l = run_project(dt, M, V1, V2, sigma, ro, 1, rows32=f)
        for lay in layouts:
            tag = "R={} n={} B={} ldm=n+{} off={} {}".format(R, n, B, lay[0], lay[1], sc.dt_name(dt))
            assert same_bits(run_gram(dt, M, rows32=f, layout=lay, what=tag), ref_row), tag
            assert same_bits(run_gram(dt, M, V1, rows32=f, layout=lay, what=tag), ref_rot), tag
            for rlay in ((0, 0), lay, (lay[0] + 1, (lay[1] + 1) % 4)):
                r, l = run_project(dt, M, V1, V2, sigma, ro, 1, rows32=f, m_layout=lay, r_layout=rlay, ldl_extra=lay[0], what=tag)
                assert same_bits(r, ref_r) and same_bits(l, ref_l), (tag, rlay)
    for rows, n in ((65, 33), (1000, 64)):
        Mr, V1, V2, sigma, _ = sc.random_batch(2, n, rows, dt)
        M = tall(Mr)
        ro = n // 2
        ref_g, ref_rg = run_colgram(dt, M), run_colgram(dt, M, V1)
        ref_l, ref_r = run_colproject(dt, M, V1, V2, sigma, ro, 1)
        for lay in ((4, 0), (_odd(n), 0), (0, 1), (_odd(n), 2), (4, 3)):
            tag = "tall rows={} n={} ldm=n+{} off={} {}".format(rows, n, lay[0], lay[1], sc.dt_name(dt))
            assert same_bits(run_colgram(dt, M, layout=lay, what=tag), ref_g) and same_bits(run_colgram(dt, M, V1, layout=lay, what=tag), ref_rg), tag
            l, r = run_colproject(dt, M, V1, V2, sigma, ro, 1, layout=lay, l_layout=(lay[0], lay[1]), ldr_extra=lay[0], what=tag)
            assert same_bits(l, ref_l) and same_bits(r, ref_r), tag


# ------------------------------------------------------------------ flags, against the truth
@DT
def test_rows32_generic_instances(dt):
    """B = 5 (below the lean threshold), rows 32.. of the flagged items NaN: never loaded, counted as zero."""
    f = [1, 0, 1, 1, 0]
    for R, n in ((64, 208), (37, 65)):
        M, V1, V2, sigma, _ = sc.random_batch(5, R, n, dt)
        M = M.clone()
        M[torch.tensor(f).bool(), 32:] = NAN
        tag = "rows32 R={} n={} {}".format(R, n, sc.dt_name(dt))
        assert_within(run_gram(dt, M, rows32=f).double().sum(dim=1), *sc.gram_truth_and_bound(M, None, dt, 1, f), "rowgram " + tag)
        assert_within(run_gram(dt, M, V1, rows32=f).double().sum(dim=1), *sc.gram_truth_and_bound(M, V1, dt, 1, f), "rotgram " + tag)
        for ro, v1, scale in ((R // 2, V1, 1), (R, V1, 0), (5, None, 1), (33, None, 0)):
            got = run_project(dt, M, v1, V2, sigma, ro, scale, rows32=f, what=tag)
            check_project(got, sc.project_truth_and_bounds(M, v1, V2, sigma, ro, scale, dt, rows32=f), "project {} ro={}".format(tag, ro))


@DT
def test_rows32_is_ignored_at_32_rows(dt):
    """R = 32 with every flag set: there are no rows 32.., every row is read."""
    M, V1, V2, sigma, _ = sc.random_batch(3, 32, 65, dt)
    f = [1, 1, 1]
    tag = "rows32 at R=32 " + sc.dt_name(dt)
    assert_within(run_gram(dt, M, rows32=f).double().sum(dim=1), *sc.gram_truth_and_bound(M, None, dt, 1), "rowgram " + tag)
    assert_within(run_gram(dt, M, V1, rows32=f).double().sum(dim=1), *sc.gram_truth_and_bound(M, V1, dt, 1), "rotgram " + tag)
    got = run_project(dt, M, V1, V2, sigma, 32, 1, rows32=f, what=tag)
    check_project(got, sc.project_truth_and_bounds(M, V1, V2, sigma, 32, 1, dt), "project " + tag)


@functools.lru_cache(maxsize=None)
def _lean_inputs(n):
    """(M [256, 64, n] fp32 with NaN rows 32.. in the flagged items, flags: every item but 3 and 200, V1, V2, sigma)."""
    M, V1, V2, sigma, sigma1 = sc.random_batch(LEAN_B, 64, n, torch.float32)
    f = [0 if b in (3, 200) else 1 for b in range(LEAN_B)]
    M = M.clone()
    M[torch.tensor(f).bool(), 32:] = NAN
    return M, f, V1, V2, sigma, sigma1


@pytest.mark.parametrize("n", [41, 208])
def test_rows32_lean_instances(n):
    """fp32, 256 items: the lean builds take the flagged items, the generic instance the two others -- all against the truth."""
    dt = torch.float32
    M, f, V1, V2, sigma, _ = _lean_inputs(n)
    tag = "lean n={}".format(n)
    assert_within(run_gram(dt, M, rows32=f).double().sum(dim=1), *sc.gram_truth_and_bound(M, None, dt, 1, f), "rowgram " + tag)
    for k, ro in enumerate((1, 16, 17, 32)):
        v1, scale = ((V1, 1), (None, 0), (V1, 0), (None, 1))[k]
        got = run_project(dt, M, v1, V2, sigma, ro, scale, rows32=f, ldl_extra=k, what=tag)
        check_project(got, sc.project_truth_and_bounds(M, v1, V2, sigma, ro, scale, dt, rows32=f), "project {} ro={}".format(tag, ro))


@DT
def test_rotgram_skip(dt):
    """Skipped items keep the sentinel in every part of G; the others are right."""
    skip = [0, 1, 0, 1, 1]
    for R, n in ((64, 1000), (37, 65)):
        M, V1, _, _, _ = sc.random_batch(5, R, n, dt)
        parts = sc.pick_split(n, 5)
        got = run_gram(dt, M, V1, skip=skip, what="rotgram skip")
        live = [b for b in range(5) if not skip[b]]
        assert is_sentinel(got[[b for b in range(5) if skip[b]]])
        G, bound = sc.gram_truth_and_bound(M, V1, dt, parts)
        assert_within(got[live].double().sum(dim=1), G[live], bound[live], "rotgram skip R={} n={} {}".format(R, n, sc.dt_name(dt)))


@DT
@pytest.mark.parametrize("rows,parts", [(65, 1), (1000, 3)])
@pytest.mark.parametrize("rotated", [False, True], ids=["plain", "rotated"])
def test_colgram_skip(dt, rows, parts, rotated):
    """`skip` as ttr_rotgram's: G of a skipped item is not written -- with one part, and with several, where the reduction of
    the partials must leave the item alone as well (its partials were never written: the workspace is NaN here)."""
    skip = [1, 0, 0, 1, 0]
    n = 48
    assert sc.col_split(rows, 5) == parts
    Mr, V1, _, _, _ = sc.random_batch(5, n, rows, dt)
    M = tall(Mr)
    v1 = V1 if rotated else None
    got = run_colgram(dt, M, v1, skip=skip, what="colgram skip")
    live = [b for b in range(5) if not skip[b]]
    assert is_sentinel(got[[b for b in range(5) if skip[b]]]), "G of a skipped item was written"
    G, bound = sc.colgram_truth_and_bound(M, v1, dt, parts)
    assert_within(got[live], G[live], bound[live], "colgram skip rows={} {}".format(rows, sc.dt_name(dt)))


def _flat_case(B, R, n, dt, flat, rows32=None):
    M, V1, V2, sigma, sigma1 = (t.clone() for t in sc.random_batch(B, R, n, dt))
    fb = torch.tensor(flat).bool()
    V2[fb] = NAN          # a pass-through item's V2 and sigma are not loaded
    sigma[fb] = NAN
    if rows32 is not None:
        M[torch.tensor(rows32).bool(), 32:] = NAN
    return M, V1, V2, sigma, sigma1


@DT
@pytest.mark.parametrize("R", [64, 37])
def test_flat_generic_instances(dt, R):
    """Mixed flags in one batch: flagged items take U = V1[:, :ro] and their scales from sigma1 (one rounding in `left`)."""
    flat = [1, 0, 1, 0, 0]
    n = 65
    M, V1, V2, sigma, sigma1 = _flat_case(5, R, n, dt, flat)
    for ro, scale in ((R // 2, 1), (R, 1), (17, 0)):
        tag = "flat R={} ro={} scale={} {}".format(R, ro, scale, sc.dt_name(dt))
        got = run_project(dt, M, V1, V2, sigma, ro, scale, flat=flat, sigma1=sigma1, what=tag)
        check_project(got, sc.project_truth_and_bounds(M, V1, V2, sigma, ro, scale, dt, flat=flat, sigma1=sigma1), "project " + tag)
    # flat given with V1 = NULL is ignored: every item reads its own V2 and sigma
    M, V1, V2, sigma, sigma1 = sc.random_batch(5, R, n, dt)
    got = run_project(dt, M, None, V2, sigma, 9, 1, flat=flat, sigma1=sigma1, what="flat without V1")
    check_project(got, sc.project_truth_and_bounds(M, None, V2, sigma, 9, 1, dt), "project flat without V1 R={} {}".format(R, sc.dt_name(dt)))


def test_flat_lean_instances():
    """fp32, 256 items of 64 rows: flat x rows32 in every combination in one batch, the lean and the generic instance side by side."""
    dt, B, n = torch.float32, LEAN_B, 41
    flat = [(b // 2) % 2 for b in range(B)]
    rows32 = [b % 2 for b in range(B)]
    M, V1, V2, sigma, sigma1 = _flat_case(B, 64, n, dt, flat, rows32)
    for ro, scale in ((32, 1), (17, 0), (1, 1)):
        tag = "flat lean ro={} scale={}".format(ro, scale)
        got = run_project(dt, M, V1, V2, sigma, ro, scale, rows32=rows32, flat=flat, sigma1=sigma1, what=tag)
        check_project(got, sc.project_truth_and_bounds(M, V1, V2, sigma, ro, scale, dt, rows32=rows32, flat=flat, sigma1=sigma1),
                      "project " + tag)


@DT
def test_sigma_null_and_scale_right(dt):
    """sigma = NULL: no scaling whatever scale_right would say (the entry refuses scale_right = 1 without sigma); scale_right = 0
    with sigma given: sigma is not used; a sigma below the smallest normal: exact zeros in its row of `right`."""
    h = _hip()
    R, n, ro = 37, 65, 20
    M, V1, V2, sigma, _ = sc.random_batch(2, R, n, dt)
    plain = sc.project_truth_and_bounds(M, V1, V2, None, ro, 0, dt)
    check_project(run_project(dt, M, V1, V2, None, ro, 0, what="sigma NULL"), plain, "project sigma NULL " + sc.dt_name(dt))
    snan = torch.full_like(sigma, NAN)
    check_project(run_project(dt, M, V1, V2, snan, ro, 0, what="scale_right 0"), plain, "project scale_right=0 " + sc.dt_name(dt))
    sz = sigma.clone()
    sz[:, 1] = sc.tiny(dt) / 4
    sz[:, 3] = 0.0
    got = run_project(dt, M, V1, V2, sz, ro, 1, what="dead sigma")
    check_project(got, sc.project_truth_and_bounds(M, V1, V2, sz, ro, 1, dt), "project dead sigma " + sc.dt_name(dt))
    assert not got[0][:, 1].any() and not got[0][:, 3].any()
    Mt = tall(M)
    got = run_colproject(dt, Mt, V1, V2, sz, ro, 1, what="dead sigma")
    check_colproject(got, sc.colproject_truth_and_bounds(Mt, V1, V2, sz, ro, 1, dt), "colproject dead sigma " + sc.dt_name(dt))
    check_colproject(run_colproject(dt, Mt, V1, V2, None, ro, 0, what="sigma NULL"),
                     sc.colproject_truth_and_bounds(Mt, V1, V2, None, ro, 0, dt), "colproject sigma NULL " + sc.dt_name(dt))
    # scale_right = 1 without sigma is refused, outputs untouched
    m, v1, v2 = dev(M), dev(V1), dev(V2)
    r = Padded((2, ro, n), dt, n, ro * n, SENTINEL, DEV)
    rc = raw("ttr_project_flat", h.dtype_code(dt), R, n, ro, 2, m.data_ptr(), n, R * n, v1.data_ptr(), R, R * R, v2.data_ptr(), R, R * R, None, 0, 1,
             r.ptr(), r.ld, r.stride, None, ro, R * ro, None, None, None, 0)
    assert rc == h.E_INVALID
    assert_guards(r, r.buf.cpu(), "refused project", window=False)


# ------------------------------------------------------------------ TTR_KNOB_SWEEP_STAGGER
@DT
def test_stagger_knob(dt):
    """0: columns in order; 1 (default): ttr_project starts item b at step b mod steps; 2: the Gram kernels as well.  The
    projection's columns are independent: the same bits at all three.  The Gram sums: the same bits at 0 and 1, within the
    bound at 2 (another summation order)."""
    h = _hip()
    B, n = 5, 1000
    for R, ro in ((64, 32), (37, 20)):
        M, V1, V2, sigma, _ = sc.random_batch(B, R, n, dt)
        parts = sc.pick_split(n, B)
        out = {}
        for v in (0, 1, 2):
            with knob(h.KNOB_SWEEP_STAGGER, v):
                out[v] = (run_gram(dt, M), run_gram(dt, M, V1), run_project(dt, M, V1, V2, sigma, ro, 1))
        tag = "stagger R={} {}".format(R, sc.dt_name(dt))
        for v in (0, 2):
            assert same_bits(out[v][2][0], out[1][2][0]) and same_bits(out[v][2][1], out[1][2][1]), (tag, v)
        assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1]), tag
        check_project(out[1][2], sc.project_truth_and_bounds(M, V1, V2, sigma, ro, 1, dt), "project " + tag)
        for v in (1, 2):
            assert_within(out[v][0].double().sum(dim=1), *sc.gram_truth_and_bound(M, None, dt, parts), "rowgram {} knob {}".format(tag, v))
            assert_within(out[v][1].double().sum(dim=1), *sc.gram_truth_and_bound(M, V1, dt, parts), "rotgram {} knob {}".format(tag, v))


# ------------------------------------------------------------------ more than 65535 items: the dispatchers' slices
BIG = 65537


@DT
def test_above_the_grid_limit_every_operand_per_item(dt):
    """65537 items of 4 x 5 (two launches: 65535 + 2): every operand per item, so that a missing per-slice offset of M, V1, V2,
    sigma, sigma1, skip, flat, G, right or left shows.  Items repeat with period 7 and the flags with period 2, so the last two
    items differ from items 0 and 1 in data and in flags."""
    B, R, n, ro = BIG, 4, 5, 2
    idx = torch.arange(B) % 7
    M, V1, V2, sigma, sigma1 = (t[idx] for t in sc.random_batch(7, R, n, dt))
    flag = (torch.arange(B) % 2).to(torch.int32)
    assert int(idx[B - 2]) != 0 and int(idx[B - 1]) != 1 and flag[B - 2] != flag[0] and flag[B - 1] != flag[1]
    live = (flag == 0).nonzero().flatten()
    tag = "B=65537 " + sc.dt_name(dt)
    assert_within(run_gram(dt, M)[:, 0], *sc.gram_truth_and_bound(M, None, dt, 1), "rowgram " + tag)
    got = run_gram(dt, M, V1, skip=flag, what="rotgram " + tag)[:, 0]
    G, bound = sc.gram_truth_and_bound(M, V1, dt, 1)
    assert is_sentinel(got[flag.bool()])
    assert_within(got[live], G[live], bound[live], "rotgram skip " + tag)
    V2n, sn = V2.clone(), sigma.clone()
    V2n[flag.bool()] = NAN
    sn[flag.bool()] = NAN
    got = run_project(dt, M, V1, V2n, sn, ro, 1, flat=flag, sigma1=sigma1, what="project_flat " + tag)
    check_project(got, sc.project_truth_and_bounds(M, V1, V2n, sn, ro, 1, dt, flat=flag, sigma1=sigma1), "project_flat " + tag)
    Mt = tall(M)                                              # rows = 5, n = 4
    got = run_colgram(dt, Mt, V1, skip=flag, what="colgram " + tag)
    assert is_sentinel(got[flag.bool()])
    assert_within(got[live], G[live], bound[live], "colgram skip " + tag)
    got = run_colproject(dt, Mt, V1, V2, sigma, ro, 1, what="colproject " + tag)
    check_colproject(got, sc.colproject_truth_and_bounds(Mt, V1, V2, sigma, ro, 1, dt), "colproject " + tag)


def test_above_the_grid_limit_rows32_flags_per_item():
    """65537 items of 33 x 4 in fp32 with per-item `rows32` flags (row 32 of a flagged item is NaN) for ttr_rowgram and
    ttr_project; V1 and V2 are shared through a batch stride of 0 (the entries accept it), M, sigma, the flags and the outputs
    are per item.  Items repeat with period 7, flags with period 2: the first and the last 14 items are compared with the truth,
    every other item with its own period's bits on the device."""
    h = _hip()
    dt, B, R, n, ro = torch.float32, BIG, 33, 4, 3
    base = sc.random_batch(7, R, n, dt)
    idx = torch.arange(B) % 7
    f = (torch.arange(B) % 2).to(torch.int32)
    M = base[0][idx].clone()
    M[f.bool(), 32:] = NAN
    sigma = base[3][idx].contiguous()
    V1, V2 = base[1][3:4], base[2][5:6]
    code = h.dtype_code(dt)
    m, v1, v2, sg, fd = dev(M), dev(V1), dev(V2), dev(sigma), flags(f)
    G = torch.full((64 + B * R * R + 64,), SENTINEL, dtype=dt, device=DEV)
    call("ttr_rowgram", code, R, n, B, m.data_ptr(), n, R * n, G.data_ptr() + 64 * 4, 1, fd.data_ptr())
    assert is_sentinel(G[:64]) and is_sentinel(G[-64:])
    Gw = G[64:-64].view(B, R, R)
    right = Padded((B, ro, n), dt, n, ro * n, SENTINEL, DEV)
    left = Padded((B, R, ro), dt, ro, R * ro, SENTINEL, DEV)
    call("ttr_project", code, R, n, ro, B, m.data_ptr(), n, R * n, v1.data_ptr(), R, 0, v2.data_ptr(), R, 0, sg.data_ptr(), R, 1,
         right.ptr(), n, ro * n, left.ptr(), ro, R * ro, fd.data_ptr())
    r, l = fetch(right, "project B=65537 right"), fetch(left, "project B=65537 left")
    sel = torch.cat([torch.arange(14), torch.arange(B - 14, B)])
    fs = f[sel]
    Gt, Gb = sc.gram_truth_and_bound(M[sel], None, dt, 1, fs)
    assert_within(Gw[sel.to(DEV)], Gt, Gb, "rowgram rows32 B=65537 f32")
    truth = sc.project_truth_and_bounds(M[sel], V1.expand(28, R, R), V2.expand(28, R, R), sigma[sel], ro, 1, dt, rows32=fs)
    check_project((r[sel], l[sel]), truth, "project rows32 B=65537 f32")
    rep = (torch.arange(B) % 14).to(DEV)
    assert torch.equal(bits(Gw), bits(Gw[:14])[rep]), "an item's Gram matrix differs from its period's"
    assert same_bits(r, r[:14][rep.cpu()]) and same_bits(l, l[:14][rep.cpu()]), "an item's projection differs from its period's"


# ------------------------------------------------------------------ ttr_spectrum_flat, ttr_carry_rows32 at their thresholds
def _next(x, up, dt):
    t = torch.tensor([x], dtype=dt)
    return float(torch.nextafter(t, torch.tensor([float("inf") if up else float("-inf")], dtype=dt)))


def _spectrum_rows(n, keep, thr, dt, margin):
    """Rows of sorted sigma whose keep-th value sits on, just below and just above thr sigma_0 (margin 0: one ulp either side of
    the exact product, thr a power of two), and sigma_0 = 0."""
    rows = []
    for s0 in (1.0, 3.0, float(torch.tensor(0.7, dtype=dt)) * 2.0 ** 40, float(torch.tensor(1.3, dtype=dt)) * 2.0 ** -40):
        at = float(torch.tensor(thr * s0, dtype=dt))
        for v in ((at, _next(at, False, dt), _next(at, True, dt)) if margin == 0 else (at * (1 - margin), at * (1 + margin))):
            row = torch.full((n,), s0, dtype=torch.float64)
            row[keep - 1:] = min(v, s0)
            row[keep:] = 0.0
            rows.append(row)
    rows.append(torch.zeros(n, dtype=torch.float64))
    return torch.stack(rows).to(dt)


@DT
@pytest.mark.parametrize("batch", [1, 300])
def test_spectrum_flat_thresholds(dt, batch):
    h = _hip()
    code = h.dtype_code(dt)
    for n in (1, 5, 64):
        for keep in sorted({1, n}):
            for thr, margin in ((0.125, 0), (0.5, 0), (1.0, 0), (0.3, 2.0 ** -10)):
                rows = _spectrum_rows(n, keep, thr, dt, margin)
                want_all = sc.spectrum_flat_rule(rows, keep, thr)
                if keep > 1 and thr < 1:
                    assert 0 < int(want_all.sum()) < len(rows)           # both outcomes occur
                pick = (torch.arange(batch) * 5 + 1) % len(rows) if batch > 1 else torch.tensor([len(rows) - 3])   # (one item: a "just below")
                s = Padded.of(rows[pick][None], 3, 0, NAN, DEV)           # [1, batch, n] with stride_sigma = n + 3
                out = torch.full((batch + 2,), -7, dtype=torch.int32, device=DEV)
                call("ttr_spectrum_flat", code, n, batch, s.ptr(), s.ld, keep, thr, 0, 0.0, None, out.data_ptr() + 4, None)
                assert out[0] == -7 and out[-1] == -7
                assert out[1:-1].cpu().tolist() == want_all[pick].tolist(), (n, keep, thr, margin)
        # keep > n is refused, the flags untouched
        out = torch.full((batch,), -7, dtype=torch.int32, device=DEV)
        s = dev(torch.ones(batch, n, dtype=dt))
        assert raw("ttr_spectrum_flat", code, n, batch, s.data_ptr(), n, n + 1, 0.125, 0, 0.0, None, out.data_ptr(), None) == h.E_INVALID
        assert bool((out == -7).all())


@DT
def test_carry_rows32_thresholds(dt):
    """Tail energy just below and just above (c eps)^2 ||R||^2 (c = 8: the library's TTR_KNOB_QR_RANK_SKIP), in a strided R whose
    padding is NaN."""
    h = _hip()
    c, eps = 8, torch.finfo(dt).eps
    cols = 7
    items = []
    for k, scale in ((1, 1.0), (9, 2.0 ** 30), (16, 2.0 ** -30)):
        for d in (-(2.0 ** -8), 2.0 ** -8, -(2.0 ** -3), 2.0 ** -3):
            Rm = torch.zeros(64, cols, dtype=torch.float64)
            Rm[:k, 2] = scale                                           # ||top||^2 = k scale^2
            Rm[40 + (k % 5), 5] = c * eps * (k ** 0.5) * scale * (1 + d)
            items.append(Rm)
    Rm = torch.stack(items).to(dt)
    want = sc.carry_rows32_rule(Rm, c, dt)
    assert want.tolist() == [1, 0, 1, 0] * 3
    p = Padded.of(Rm, 3, 5, NAN, DEV, 1)
    out = torch.full((len(items) + 2,), -7, dtype=torch.int32, device=DEV)
    call("ttr_carry_rows32", h.dtype_code(dt), cols, len(items), p.ptr(), p.ld, p.stride, out.data_ptr() + 4)
    assert out[0] == -7 and out[-1] == -7
    assert out[1:-1].cpu().tolist() == want.tolist()


# ------------------------------------------------------------------ refusals leave the outputs untouched
@DT
def test_refusals_leave_the_outputs_untouched(dt):
    h = _hip()
    code = h.dtype_code(dt)
    es = 4 if dt == torch.float32 else 8
    big = dev(torch.zeros(2 * 66 * 66, dtype=dt))              # any claimed operand fits: nothing could leave it
    out = Padded((1, 1, 2 * 66 * 66), dt, 2 * 66 * 66, 0, SENTINEL, DEV)
    out2 = Padded((1, 1, 2 * 66 * 66), dt, 2 * 66 * 66, 0, SENTINEL, DEV)
    b, o, o2 = big.data_ptr(), out.ptr(), out2.ptr()

    def untouched(what):
        assert_guards(out, out.buf.cpu(), what, window=False)
        assert_guards(out2, out2.buf.cpu(), what, window=False)

    U, I, W = h.E_UNSUPPORTED, h.E_INVALID, h.E_WORKSPACE
    assert raw("ttr_rowgram", code, 65, 8, 1, b, 8, 65 * 8, o, 1, None) == U
    assert raw("ttr_rotgram", code, 65, 8, 1, b, 8, 65 * 8, b, 65, 65 * 65, o, 1, None, None) == U
    assert raw("ttr_rowgram", code, 8, 8, 1, b, 8, 64, o, 0, None) == I
    assert raw("ttr_rotgram", code, 8, 8, 1, b, 8, 64, b, 8, 64, o, 0, None, None) == I
    untouched("gram refusals")

    def project(R, ro):
        return raw("ttr_project", code, R, 8, ro, 1, b, 8, R * 8, b, R, R * R, b, R, R * R, b, R, 1, o, 8, 8 * max(ro, 1), o2, max(ro, 1),
                   R * max(ro, 1), None)

    assert project(65, 8) == U and project(8, 9) == U and project(8, 0) == U and project(64, 65) == U
    untouched("project refusals")
    assert raw("ttr_colgram", code, 8, 65, 1, b, 65, 8 * 65, None, 0, 0, o, None, 0, None) == U

    def colproject(n, ro):
        return raw("ttr_colproject", code, 8, n, ro, 1, b, n, 8 * n, b, n, n * n, b, n, n * n, b, n, 1, o, max(ro, 1), 8 * max(ro, 1), o2, n,
                   max(ro, 1) * n)

    assert colproject(65, 8) == U and colproject(8, 9) == U and colproject(8, 0) == U
    untouched("col refusals")
    # a colgram workspace one byte short (rows = 1000, two items: three parts)
    rows, n, B = 1000, 8, 2
    wsb = int(h.lib().ttr_colgram_workspace_bytes(code, rows, n, B))
    assert wsb == 3 * B * n * n * es
    M = dev(sc.random_batch(B, n, rows, dt)[0].transpose(1, 2))
    ws = nan_bytes(wsb)
    assert raw("ttr_colgram", code, rows, n, B, M.data_ptr(), n, rows * n, None, 0, 0, o, ws.data_ptr(), wsb - 1, None) == W
    assert raw("ttr_colgram", code, rows, n, B, M.data_ptr(), n, rows * n, None, 0, 0, o, None, 0, None) == W
    untouched("workspace refusals")
    assert bool((ws == 0xFF).all())
    assert raw("ttr_colgram", code, rows, n, B, M.data_ptr(), n, rows * n, None, 0, 0, o, ws.data_ptr(), wsb, None) == 0

"""The streaming kernels (ttr_vec.hip: norm, scale_cols, mask_cols, pow2_normalize, scale_batch; ttr_cp.hip: hadamard,
krp_contract, core_kron) through the raw C ABI on a real MI355X, at the sizes where each takes another path: below, at and above
a block of 256, past the block cap of its grid-stride loop, the unroll tail, a leading dimension larger than the row.

Method as for the GEMM (gemm_cases.py): inputs are views inside NaN-filled buffers, outputs inside sentinel-filled buffers with
guard elements on either side; everything outside the output keeps its bits.  Bounds, with u the unit roundoff of the dtype:
  norm          2 u ref    (the squares are summed in double: only the final rounding counts, u; the other u is slack for the
                           double sum and the wrapper's second stage).  ref is the exact sum of squares (`exact_norms`), its
                           square root taken at 50 digits: for fp64 a plain fp64 reference would err as much as the kernel
  scale MUL     u |x s|    (one correctly rounded product);  DIV  2 u |x / s|  (one division; the second u because the rounding
                           of the fp32 division under the build's flags is not established)
  hadamard, core_kron, pow2 scaling: one exact or correctly rounded operation -- equal bits
  krp_contract  2 (J + 2) u sum_j |T||B|   (J products summed in any order, Higham section 3.1; exact on integer data)
"""
import decimal
import math

import pytest
import torch

import gemm_cases as gc
from gemm_cases import SCALE_DIV, SCALE_MUL, SENTINEL, Padded

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
DT = pytest.mark.parametrize("dt", gc.DTYPES, ids=["f32", "f64"])


def _hip():
    from tntorch_amd import _hip

    _hip.lib()
    return _hip


def call(name, *args):
    h = _hip()
    rc = getattr(h.lib(), name)(*args, h._stream())
    assert rc == 0, (name, rc, h.lib().ttr_last_error())
    torch.cuda.synchronize()


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a.contiguous()), bits(b.contiguous()))


def rel_ratio(group, got, truth, k, dt, what):
    """|got - truth| <= k u |truth| in every element; prints the largest err / bound."""
    bound = k * gc.unit(dt) * truth.abs()
    r, idx = gc.worst_ratio(got, truth, bound)
    print(f"ratio[{group}] {r:.3e} at {idx}: {what}")
    gc.assert_within(got, truth, bound, what)


def exact_norms(x):
    """sqrt(sum x[b]^2) per row as decimal.Decimal at 50 digits, from the EXACT sum of squares: every square is split into
    hi + lo without error (Veltkamp / Dekker; fp32 squares are exact in double, lo = 0), math.fsum adds the pieces with one
    rounding, and a second fsum returns what that rounding lost."""
    x = x.double()
    c = 134217729.0 * x                                   # 2^27 + 1
    xh = c - (c - x)
    xl = x - xh
    hi = x * x
    lo = ((xh * xh - hi) + 2.0 * xh * xl) + xl * xl
    out = []
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        for h_, l_ in zip(hi.tolist(), lo.tolist()):
            s = math.fsum(h_ + l_)
            rest = math.fsum(h_ + l_ + [-s])
            out.append((decimal.Decimal(s) + decimal.Decimal(rest)).sqrt())
    return out


def norm_ratio(group, got, x, dt, what):
    """|got[b] - ||x[b]||| <= 2 u ||x[b]|| against the exact norm; prints the largest err / bound."""
    worst = 0.0
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        for b, ref in enumerate(exact_norms(x)):
            v = got[b].item()
            assert math.isfinite(v), (what, b, v)
            err, bound = abs(decimal.Decimal(v) - ref), decimal.Decimal(2.0 * gc.unit(dt)) * ref
            r = float(err / bound) if bound > 0 else (0.0 if err == 0 else math.inf)
            worst = max(worst, r)
    print(f"ratio[{group}] {worst:.3e}: {what}")
    assert worst <= 1.0, f"{what}: |err| = {worst:.3g} x the bound 2 u ref"


def vec(x, stride_extra=3, fill=NAN, offset=0):
    """[B, count] on the device, items count + stride_extra apart."""
    return Padded.of(x[:, None, :], 0, stride_extra, fill, DEV, offset)


def out_like(B, r, c, dt, ld_extra=5, stride_extra=7):
    return Padded((B, r, c), dt, c + ld_extra, r * (c + ld_extra) + stride_extra, SENTINEL, DEV)


def fetch(p, what):
    """The output window of p on the CPU, after checking that nothing around it was written."""
    buf = p.buf.cpu()
    gc.assert_guards(p, buf, what)
    return p.view(buf).clone()


def draw(shape, dt, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, dtype=torch.float64, generator=g).to(dt)


# ------------------------------------------------------------------ ttr_norm
@DT
@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 255, 256, 257, 1023])
def test_norm(count, dt):
    h = _hip()
    B = 3
    x = draw((B, count), dt, 100 + count)
    x[1] *= 2.0 ** 40
    if count > 1:
        x[2, 1::2] = 0
    xp, out = vec(x), out_like(1, 1, B, dt)
    call("ttr_norm", h.dtype_code(dt), count, B, xp.ptr(), xp.stride, out.ptr())
    norm_ratio("norm", fetch(out, f"norm {count}")[0, 0], x, dt, f"norm count={count} {dt}")


@DT
def test_norm_of_huge_entries_and_of_zero(dt):
    """Entries whose squares overflow the dtype's range (fp32: 1e25^2) but not the double accumulator; an all-zero item gives 0."""
    h = _hip()
    big = 1e25 if dt == torch.float32 else 1e150
    x = draw((3, 257), dt, 7).sign() * big
    x[1] = 0
    assert not torch.isfinite(x[0] * x[0]).any() or dt == torch.float64
    xp, out = vec(x), out_like(1, 1, 3, dt)
    call("ttr_norm", h.dtype_code(dt), 257, 3, xp.ptr(), xp.stride, out.ptr())
    got = fetch(out, "norm huge")[0, 0]
    assert torch.isfinite(got).all() and got[1] == 0 and not torch.signbit(got[1])
    norm_ratio("norm", got, x, dt, f"norm huge {dt}")


@DT
@pytest.mark.parametrize("count,two_stage", [(1 << 20, True), (3 << 19, True), ((1 << 20) + 1, False)])
def test_norm_wrapper_two_stage_path(count, two_stage, dt):
    """_hip.norm splits one long vector (count >= 2^20, a power-of-two divisor) into chunk norms and takes the norm of those: two
    ttr_norm calls instead of one, both within the bound."""
    h = _hip()
    x = draw((1, count), dt, count % 1000)
    xd = x.to(DEV)
    h.prof_enable(True)
    try:
        h.prof_collect()
        got = h.norm(xd).cpu()
        torch.cuda.synchronize()
        calls = h.prof_collect()["misc"]["launches"]
    finally:
        h.prof_enable(False)
    assert calls == (2 if two_stage else 1)
    norm_ratio("norm-wrapper", got, x, dt, f"norm wrapper count={count} {dt}")


# ------------------------------------------------------------------ ttr_scale_cols
@DT
@pytest.mark.parametrize("mode", [SCALE_MUL, SCALE_DIV], ids=["mul", "div"])
@pytest.mark.parametrize("rows,cols", [(750, 800), (1, 1), (3, 257)])   # 750 x 800 > 2048 blocks x 256 threads: the grid-stride loop
def test_scale_cols(rows, cols, mode, dt):
    h = _hip()
    B = 2
    assert (rows, cols) != (750, 800) or rows * cols > 2048 * 256
    x = draw((B, rows, cols), dt, rows + cols) * 2.0 ** -4      # (|x| < 1: the quotient by the smallest normal is finite)
    g = torch.Generator().manual_seed(cols)
    s = ((torch.rand((B, cols), dtype=torch.float64, generator=g) + 0.5) * torch.where(torch.rand((B, cols), generator=g) < 0.5, -1.0, 1.0)).to(dt)
    dead = torch.zeros((B, cols), dtype=torch.bool)
    if mode == SCALE_DIV and cols >= 6:
        thr = gc.threshold_scales(dt)
        s[0, :6], s[1, -6:] = thr, thr.flip(0)
        dead = s.abs() < torch.finfo(dt).tiny
        assert dead.sum() == 8
    xp = Padded.of(x, 3, 5, NAN, DEV)
    sp = vec(s)
    out = out_like(B, rows, cols, dt)
    call("ttr_scale_cols", h.dtype_code(dt), rows, cols, B, xp.ptr(), xp.ld, xp.stride, sp.ptr(), sp.stride, mode, out.ptr(), out.ld,
         out.stride)
    got = fetch(out, f"scale_cols {rows}x{cols}")
    sd = s.double()[:, None, :]
    if mode == SCALE_MUL:
        truth, k = x.double() * sd, 1
    else:
        truth, k = torch.where(dead[:, None, :], torch.zeros((), dtype=torch.float64), x.double() / torch.where(dead[:, None, :], torch.ones_like(sd), sd)), 2
        assert (got[dead[:, None, :].expand_as(got)] == 0).all(), "a scale below the smallest normal must give exactly 0"
    assert torch.isfinite(truth).all()
    rel_ratio("scale_cols", got, truth, k, dt, f"scale_cols {rows}x{cols} mode {mode} {dt}")


# ------------------------------------------------------------------ ttr_mask_cols
def _mask_case(rows, cols, keep, dt):
    h = _hip()
    B = len(keep)
    x = draw((B, rows, cols), dt, rows * cols)
    x[x == 0] = 1.0
    xp = Padded.of(x, 3, 5, SENTINEL, DEV)               # in place: the padding is a guard as well
    want = xp.buf.cpu()
    for b, k in enumerate(keep):
        xp.view(want)[b, :, max(k, 0):] = 0.0
    kd = torch.tensor([-77] + list(keep) + [-77], dtype=torch.int32, device=DEV)
    call("ttr_mask_cols", h.dtype_code(dt), rows, cols, B, xp.ptr(), xp.ld, xp.stride, kd.data_ptr() + 4)
    got = xp.buf.cpu()
    assert same_bits(got, want), f"mask_cols {rows}x{cols} keep {keep}: {int((bits(got) != bits(want)).sum())} elements differ (masked entries are +0, all others keep their bits)"
    assert kd.cpu().tolist() == [-77] + list(keep) + [-77]


@DT
@pytest.mark.parametrize("rows,cols", [(300, 900), (5, 7)])   # 300 x 900 > 1024 blocks x 256 threads: the grid-stride loop
def test_mask_cols(rows, cols, dt):
    assert (rows, cols) != (300, 900) or rows * cols > 1024 * 256
    _mask_case(rows, cols, [0, 1, cols - 1, cols, cols + 5], dt)


@DT
@pytest.mark.parametrize("rows,cols", [(300, 900), (5, 7)])
def test_mask_cols_negative_keep_counts_as_zero(rows, cols, dt):
    """keep[b] < 0 is clamped in the kernel (it used to start writing keep[b] elements before each row): the whole item is
    zeroed, nothing around it is touched."""
    _mask_case(rows, cols, [-1, cols, -5, 2, -2 ** 31], dt)


# ------------------------------------------------------------------ ttr_pow2_normalize / ttr_scale_batch
@DT
@pytest.mark.parametrize("count", [1, 1023, 1024, 1025, (1 << 20) + 5])   # scale_batch: 1024 elements per block, 1024 blocks at most
def test_pow2_normalize_and_scale_batch(count, dt):
    h = _hip()
    B = 4
    x = draw((B, count), dt, count % 977)
    x[x == 0] = 1.0
    x[1] *= 1e20 if dt == torch.float64 else 1e15
    x[2] *= 1e-20 if dt == torch.float64 else 1e-15
    x[3] = 0
    xp, y = vec(x), Padded((B, 1, count), dt, count, count + 7, SENTINEL, DEV)
    ed = torch.full((B + 2,), -77, dtype=torch.int32, device=DEV)
    acc = torch.full((B + 2,), 3, dtype=torch.int32, device=DEV)
    call("ttr_pow2_normalize", h.dtype_code(dt), count, B, xp.ptr(), xp.stride, y.ptr(), y.stride, ed.data_ptr() + 4, acc.data_ptr() + 4)
    want_e = torch.frexp(x.double().square().sum(dim=1).sqrt())[1].to(torch.int32)
    want_e[3] = 0
    e = ed.cpu()
    assert e[0] == -77 and e[-1] == -77 and torch.equal(e[1:-1], want_e)
    assert acc.cpu().tolist() == [3] + (want_e + 3).tolist() + [3]
    yn = fetch(y, f"pow2_normalize {count}")[:, 0]
    assert same_bits(yn, torch.ldexp(x, -want_e[:, None])), "x * 2^-e is exact"
    # exponents only
    ed.fill_(-77)
    call("ttr_pow2_normalize", h.dtype_code(dt), count, B, xp.ptr(), xp.stride, None, 0, ed.data_ptr() + 4, None)
    assert ed.cpu().tolist() == [-77] + want_e.tolist() + [-77]
    # the round trip through ttr_scale_batch gives x back bit for bit
    back = Padded((B, 1, count), dt, count, count + 5, SENTINEL, DEV)
    call("ttr_scale_batch", h.dtype_code(dt), count, B, y.ptr(), y.stride, None, 0, ed.data_ptr() + 4, 1, back.ptr(), back.stride)
    assert same_bits(fetch(back, f"scale_batch {count}")[:, 0], x)
    # one scalar for the batch (stride_scale = 0), one scale per item
    for s, ss in ((torch.tensor([-2.5], dtype=dt), 0), (torch.tensor([3.0, -1.0 / 3.0, 0.7, 1.1], dtype=dt), 1)):
        back.refill()
        sd = s.to(DEV)
        call("ttr_scale_batch", h.dtype_code(dt), count, B, xp.ptr(), xp.stride, sd.data_ptr(), ss, None, 1, back.ptr(), back.stride)
        rel_ratio("scale_batch", fetch(back, f"scale_batch {count}")[:, 0], x.double() * s.double()[:, None], 1, dt,
                  f"scale_batch count={count} stride_scale={ss} {dt}")


# ------------------------------------------------------------------ ttr_hadamard
@DT
@pytest.mark.parametrize("count", [1, 255, 256, 257, 4096 * 256 + 3])   # past the cap of 4096 blocks: the grid-stride loop
def test_hadamard(count, dt):
    h = _hip()
    a, b = draw((1, count), dt, count % 991), draw((1, count), dt, count % 991 + 1)
    ap, bp = vec(a), vec(b)
    out = Padded((1, 1, count), dt, count, count, SENTINEL, DEV)
    call("ttr_hadamard", h.dtype_code(dt), count, ap.ptr(), bp.ptr(), out.ptr())
    assert same_bits(fetch(out, f"hadamard {count}")[0], a * b)


# ------------------------------------------------------------------ ttr_krp_contract
KRP_INNER = {3: (1, 3), 100: (4, 25), 255: (5, 51), 256: (2, 128), 257: (1, 257), 300: (3, 100)}   # Q R -> (Q, R)


def _krp_cases():
    for inner, (Q, R) in KRP_INNER.items():
        JS = 256 // min(inner, 256)            # the dispatcher's j slices (before its clamp to J)
        for J in sorted({1, JS, 4 * JS - 1, 4 * JS, 4 * JS + 1}):   # the four-way unrolled j loop: no tail, a tail of 3, none, of 1
            yield inner, Q, R, J


@DT
@pytest.mark.parametrize("inner,Q,R,J", list(_krp_cases()))
def test_krp_contract(inner, Q, R, J, dt):
    h = _hip()
    P = 3
    assert Q * R == inner
    g = torch.Generator().manual_seed(inner + J)
    for exact in (True, False):
        if exact:
            T, Bm = torch.randint(-3, 4, (P, J, Q, R), generator=g).to(dt), torch.randint(-3, 4, (J, R), generator=g).to(dt)
        else:
            T, Bm = draw((P, J, Q, R), dt, inner + J), draw((J, R), dt, inner + J + 1)
        tp = vec(T.reshape(1, -1))
        bp = Padded.of(Bm[None], 3, 0, NAN, DEV)
        out = Padded((1, 1, P * inner), dt, P * inner, 0, SENTINEL, DEV)
        call("ttr_krp_contract", h.dtype_code(dt), P, J, Q, R, tp.ptr(), bp.ptr(), bp.ld, out.ptr())
        what = f"krp_contract Q={Q} R={R} J={J} {dt}"
        got = fetch(out, what).reshape(P, Q, R)
        truth = torch.einsum("pjqr,jr->pqr", T.double(), Bm.double())
        if exact:
            gc.assert_exact(got, truth, what + " (integers)")
        else:
            bound = 2.0 * (J + 2) * gc.unit(dt) * torch.einsum("pjqr,jr->pqr", T.double().abs(), Bm.double().abs())
            r, idx = gc.worst_ratio(got, truth, bound)
            print(f"ratio[krp_contract] {r:.3e} at {idx}: {what}")
            gc.assert_within(got, truth, bound, what)


# ------------------------------------------------------------------ ttr_core_kron
@DT
@pytest.mark.parametrize("R2,S2", [(17, 20), (1, 1)])   # R2 S2 = 340 > 256 threads: the column loop runs twice
def test_core_kron(R2, S2, dt):
    h = _hip()
    B, R1, S1, I = 2, 2, 3, 3
    a, c = draw((B, R1, I, R2), dt, R2), draw((B, S1, I, S2), dt, S2 + 50)
    ap, cp = vec(a.reshape(1, -1)), vec(c.reshape(1, -1))
    n = B * R1 * S1 * I * R2 * S2
    out = Padded((1, 1, n), dt, n, 0, SENTINEL, DEV)
    call("ttr_core_kron", h.dtype_code(dt), B, R1, S1, I, R2, S2, ap.ptr(), cp.ptr(), out.ptr())
    want = (a[:, :, None, :, :, None] * c[:, None, :, :, None, :]).reshape(B, R1 * S1, I, R2 * S2)
    assert same_bits(fetch(out, f"core_kron {R2}x{S2}").reshape(want.shape), want)

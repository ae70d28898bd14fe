"""What the tests of ``ttr_gemm`` / ``ttr_gemm_axpby`` and of the streaming kernels (``ttr_vec.hip``, ``ttr_cp.hip``) share: shape
tables, seeded operands, the fp64 truth with its per-element bound, and the padded / guarded buffers.  Importable without a GPU.

The bound.  C = alpha * (op(A) op(B)) / rs * cs + beta * C0 is computed by the kernels as a sum of K products in the working
precision (in any order: MFMA chains, split-K partials and their reduction) followed by at most four roundings in the epilogue
(row scale, column scale, alpha, the sum with beta * C0).  With u the unit roundoff, every summation order of K terms is within
gamma_K = K u / (1 - K u) of the exact sum relative to sum |a||b| (Higham, Accuracy and Stability, section 3.1), and each epilogue
rounding adds u relative to what it rounds, so to first order
    |Chat - C| <= (K + 4) u * (|alpha| * (|op(A)| |op(B)|) / |rs| * |cs| + |beta| |C0|).
The tests use twice that: the factor 2 covers the higher-order terms (and, for fp64, the error of the fp64 truth itself, which
is another gamma_K of the same product at most).  Nothing in the bound was measured.

Exact data.  Integer operands in [-3, 3] give partial sums of magnitude <= 9 K; for K <= 32768 that is 294912 < 2^24, so every
product and every partial sum is an integer that fp32 represents: the result is exact in ANY summation order.  Scales that are
powers of two, alpha = -0.5 and beta = 2 keep it exact (they change exponents only; -0.5 P + 2 C0 needs 20 bits).  On such data a
kernel must reproduce the fp64 truth bit for bit, and a dropped / doubled k-term or a misplaced element cannot hide in a bound.
"""
import collections

import torch

DTYPES = [torch.float32, torch.float64]

SCALE_NONE, SCALE_MUL, SCALE_DIV = 0, 1, 2   # (include/ttround_hip.h: TTR_SCALE_*)
ALPHA, BETA = -0.5, 2.0
# what untouched output memory holds: finite, no integer, not a value any case produces
SENTINEL = 12345.678
GUARD = 64

Case = collections.namedtuple("Case", "M N K tA tB B")
Ops = collections.namedtuple("Ops", "A Bm C rs cs")


def unit(dt):
    return 2.0 ** -24 if dt == torch.float32 else 2.0 ** -53


def case_id(c):
    return f"{c.M}x{c.N}x{c.K}-{'T' if c.tA else 'N'}{'T' if c.tB else 'N'}-b{c.B}"


# ------------------------------------------------------------------ shape tables
_ORI = [(False, False), (True, False), (False, True), (True, True)]
# the tile-shape switch (N <= 32 && M >= 128 -> 128 x 32; M <= 32 && N >= 128 -> 32 x 128; else 64 x 64): one below, at, one above
_SWITCH_MN = [(127, 32), (128, 32), (129, 32), (128, 33), (129, 31), (32, 127), (32, 128), (32, 129), (33, 128), (31, 129)]
SWITCH_CASES = [Case(M, N, 19, False, False, 2) for M, N in _SWITCH_MN] + \
               [Case(M, N, 19, tA, tB, 2) for M, N in ((128, 32), (32, 128)) for tA, tB in _ORI[1:]]
# the 64-wide tile edge and the K step of 16 (MFMA steps of 4 inside it)
EDGE_CASES = [Case(M, N, K, False, False, 1) for M in (63, 64, 65) for N in (63, 64, 65) for K in (1, 3, 4, 5, 15, 16, 17, 33)]
SMALL_CASES = SWITCH_CASES + EDGE_CASES + [Case(1, 1, 1, False, False, 1)]
BROADCAST_CASE = Case(70, 45, 19, False, True, 3)   # strideB = 0: one B for the three items
# few tiles, long K: the 64 x 64 kernel splits K and a second kernel reduces (and applies the epilogue)
SPLIT_CASES = [Case(M, N, K, tA, False, B) for (M, N, K, tA) in ((1, 1, 2048, False), (5, 7, 2055, False), (48, 48, 4100, True))
               for B in (1, 2)]
# fp32, M, N >= 128, K >= 64, all multiples of 4: the 128 x 128-tile kernel; ragged tiles (132, 260) and K tails (68, 80, 260)
BIG_CASES = [Case(M, N, K, tA, tB, 2) for M in (128, 132, 256, 260) for N in (128, 132, 256, 260) for K in (64, 68, 80, 260)
             for tA, tB in _ORI]
BIG_NINE_ROW_TILES = Case(1156, 132, 64, False, False, 2)   # nine row tiles: one more than a round of the 8-way workgroup map
BIG_RAGGED = Case(132, 260, 68, True, False, 2)
# shapes / layouts the big kernel must decline (the 64 x 64 kernel runs): (case, lda extra, element offset of A)
BIG_FALLBACKS = {
    "M=124": (Case(124, 132, 68, False, False, 2), 4, 0),
    "M=130": (Case(130, 132, 68, False, False, 2), 4, 0),
    "K=60": (Case(132, 132, 60, False, False, 2), 4, 0),
    "lda=K+3": (Case(132, 132, 68, False, False, 2), 3, 0),
    "A+1": (Case(132, 132, 68, False, False, 2), 4, 1),
}
BIG_SPLIT_CASE = Case(256, 256, 16384, True, False, 1)
# symmetric products, (side, rows, cols) of the stored A: A^T A ("ata": cols x cols, K = rows) or A A^T ("aat": rows x rows, K = cols)
SYM_CASES = [("ata", 68, 132), ("ata", 80, 260), ("ata", 32768, 128), ("aat", 260, 96)]


def sym_case(side, rows, cols, B=1):
    """The Case of a symmetric product of the stored [rows, cols] matrix with itself."""
    return Case(cols, cols, rows, True, False, B) if side == "ata" else Case(rows, rows, cols, False, True, B)


ALL_CASES = SMALL_CASES + [BROADCAST_CASE] + SPLIT_CASES + BIG_CASES + [BIG_NINE_ROW_TILES, BIG_RAGGED, BIG_SPLIT_CASE] + \
            [v[0] for v in BIG_FALLBACKS.values()] + [sym_case(*s) for s in SYM_CASES]


# ------------------------------------------------------------------ operands
def _shapes(c):
    return ((c.B, c.K, c.M) if c.tA else (c.B, c.M, c.K)), ((c.B, c.N, c.K) if c.tB else (c.B, c.K, c.N))


def _seed(c, seed):
    return seed + 7 * c.M + 3 * c.N + c.K + 2 * c.tA + c.tB + 11 * c.B


def operands(case, dt, seed=5):
    """Ops(A, Bm, C, rs, cs) as stored (A: [B, K, M] when tA else [B, M, K]; Bm alike), drawn in fp64 and rounded to dt; the scales
    lie in [0.5, 1.5)."""
    g = torch.Generator().manual_seed(_seed(case, seed))
    sa, sb = _shapes(case)
    draw = lambda *s: torch.randn(s, dtype=torch.float64, generator=g).to(dt)  # noqa: E731
    pos = lambda *s: (torch.rand(s, dtype=torch.float64, generator=g) + 0.5).to(dt)  # noqa: E731
    return Ops(draw(*sa), draw(*sb), draw(case.B, case.M, case.N), pos(case.B, case.M), pos(case.B, case.N))


def int_operands(case, dt, seed=5):
    """The same layout with integers in [-3, 3] and power-of-two scales 2^-2 .. 2^2: every result is exact (module docstring)."""
    assert 9 * case.K < 2 ** 24, case
    g = torch.Generator().manual_seed(_seed(case, seed) + 1)
    sa, sb = _shapes(case)
    draw = lambda *s: torch.randint(-3, 4, s, generator=g).to(dt)  # noqa: E731
    pow2 = lambda *s: torch.ldexp(torch.ones(s, dtype=dt), torch.randint(-2, 3, s, generator=g))  # noqa: E731
    return Ops(draw(*sa), draw(*sb), draw(case.B, case.M, case.N), pow2(case.B, case.M), pow2(case.B, case.N))


def threshold_scales(dt):
    """[0, -0, smallest subnormal, largest subnormal, smallest normal, -smallest normal] in dt: TTR_SCALE_DIV gives exactly 0 for
    the first four and the quotient for the last two."""
    tiny = torch.tensor(torch.finfo(dt).tiny, dtype=dt)
    zero = torch.zeros((), dtype=dt)
    return torch.stack([zero, -zero, torch.nextafter(zero, tiny), torch.nextafter(tiny, zero), tiny, -tiny])


def op(x, trans):
    return x.transpose(-1, -2) if trans else x


def _scaled(P, s, mode, dt, axis):
    if mode == SCALE_NONE:
        return P
    s = s.double().unsqueeze(axis)
    if mode == SCALE_MUL:
        return P * s
    dead = s.abs() < torch.finfo(dt).tiny
    return torch.where(dead, torch.zeros_like(P), P / torch.where(dead, torch.ones_like(s), s))


def truth_and_bound(case, ops, dt, rs_mode=SCALE_NONE, cs_mode=SCALE_NONE, alpha=None, beta=None):
    """(C64, bound) [B, M, N] of the rounded operands as given: the product, the scales and the axpby in fp64, and the bound of
    the module docstring.  alpha = None: no axpby (C is overwritten)."""
    A, Bm = op(ops.A.double(), case.tA), op(ops.Bm.double(), case.tB)
    P, absP = A @ Bm, A.abs() @ Bm.abs()
    for s, mode, axis in ((ops.rs, rs_mode, 2), (ops.cs, cs_mode, 1)):
        P = _scaled(P, s, mode, dt, axis)
        absP = _scaled(absP, None if s is None else s.abs(), mode, dt, axis)
    if alpha is not None:
        C0 = ops.C.double()
        P, absP = alpha * P + (beta * C0 if beta != 0 else 0.0), abs(alpha) * absP + (abs(beta) * C0.abs() if beta != 0 else 0.0)
    return P, 2.0 * (case.K + 4) * unit(dt) * absP


def worst_ratio(got, truth, bound):
    """(max over the elements of err / bound, its index): inf where got is not finite or errs at a zero bound."""
    err = (got.double() - truth).abs()
    inf = torch.full_like(err, float("inf"))
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), inf))
    ratio = torch.where(torch.isfinite(got.double()) & ~torch.isnan(ratio), ratio, inf)
    if ratio.numel() == 0:
        return 0.0, ()
    k = ratio.reshape(-1).argmax()
    return float(ratio.reshape(-1)[k]), tuple(int(i) for i in torch.unravel_index(k, ratio.shape))


def assert_within(got, truth, bound, what=""):
    """Every element of got within its bound of truth; reports the worst element.  Returns max err / bound."""
    assert got.shape == truth.shape == bound.shape, (what, got.shape, truth.shape, bound.shape)
    r, idx = worst_ratio(got, truth, bound)
    assert r <= 1.0, (f"{what}: element {idx} is {got[idx].item()!r}, truth {truth[idx].item()!r}: "
                      f"|err| = {abs(got[idx].double().item() - truth[idx].item()):.3e} = {r:.3g} x its bound {bound[idx].item():.3e}")
    return r


def assert_exact(got, truth, what=""):
    """Exact data: got equals the fp64 truth in every element."""
    g = got.double()
    if not torch.equal(g, truth):
        bad = (g != truth).nonzero()
        idx = tuple(int(i) for i in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {g.numel()} elements differ from the exact result, first {idx}: "
                             f"{g[idx].item()!r} instead of {truth[idx].item()!r}")


# ------------------------------------------------------------------ padded operands, guarded outputs
class Padded:
    """A [B, r, c] matrix inside a flat buffer filled with `fill`: GUARD elements, `offset` more, the items at distance `stride`
    with leading dimension `ld`, GUARD elements.  Inputs are padded with NaN (a kernel that reads past its extents returns NaN),
    outputs with SENTINEL (`assert_guards`)."""

    def __init__(self, shape, dt, ld, stride, fill, device="cpu", offset=0, guard=GUARD):
        B, r, c = shape
        assert ld >= c and (B <= 1 or stride == 0 or stride >= (r - 1) * ld + c)
        self.shape, self.ld, self.stride, self.start, self.fill = (B, r, c), ld, stride, guard + offset, fill
        n = self.start + max(B - 1, 0) * stride + max(r - 1, 0) * ld + c + guard
        self.buf = torch.full((n,), fill, dtype=dt, device=device)

    @classmethod
    def of(cls, mat, ld_extra, stride_extra, fill, device="cpu", offset=0):
        B, r, c = mat.shape
        ld = c + ld_extra
        p = cls((B, r, c), mat.dtype, ld, r * ld + stride_extra, fill, device, offset)
        p.view().copy_(mat)
        return p

    def view(self, buf=None):
        buf = self.buf if buf is None else buf
        return buf.as_strided(self.shape, (self.stride, self.ld, 1), self.start)

    def ptr(self):
        return self.buf.data_ptr() + self.start * self.buf.element_size()

    def refill(self, mat=None):
        self.buf.fill_(self.fill)
        if mat is not None:
            self.view().copy_(mat)


def assert_guards(p, buf, what="", window=True):
    """Every element of `buf` (a copy of p.buf after a kernel ran) outside p's [B, r, c] window still holds p.fill bit for bit
    (window = False: the window's elements too -- a call that must write nothing)."""
    bits = torch.int32 if buf.dtype == torch.float32 else torch.int64
    b = buf.detach().cpu().clone()
    if window:
        p.view(b).fill_(p.fill)
    bad = (b.view(bits) != torch.full_like(b, p.fill).view(bits)).nonzero()
    assert bad.numel() == 0, (f"{what}: {bad.shape[0]} elements outside the output window were written, first at flat offset "
                              f"{int(bad[0]) - p.start} from the window's start (ld {p.ld}, stride {p.stride}): {b[int(bad[0])].item()!r}")

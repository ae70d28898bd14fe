"""The helpers of gemm_cases.py cannot hide a failure (CPU): the reference alone passes the bound, and one dropped k-term, one
element left at the sentinel or one write outside the output window fails it."""
import pytest
import torch

import gemm_cases as gc

# one per kernel family: 64 x 64 tiles with ragged edges, a split-K shape, a big-tile shape
REPRESENTATIVE = [gc.Case(65, 63, 17, False, False, 2), gc.Case(5, 7, 2055, False, False, 2), gc.BIG_RAGGED]
IDS = [gc.case_id(c) for c in REPRESENTATIVE]


def _cpu_result(case, ops, dt, rs_mode=gc.SCALE_NONE, cs_mode=gc.SCALE_NONE, alpha=None, beta=None):
    """The same operation as plain torch arithmetic in dt on the CPU."""
    P = gc.op(ops.A, case.tA) @ gc.op(ops.Bm, case.tB)
    if rs_mode == gc.SCALE_DIV:
        P = P / ops.rs[:, :, None]
    if cs_mode == gc.SCALE_MUL:
        P = P * ops.cs[:, None, :]
    if alpha is not None:
        P = alpha * P + beta * ops.C
    return P


@pytest.mark.parametrize("dt", gc.DTYPES)
@pytest.mark.parametrize("case", REPRESENTATIVE, ids=IDS)
def test_the_cpu_product_in_the_same_precision_is_within_the_bound(case, dt):
    ops = gc.operands(case, dt)
    for kw in ({}, {"rs_mode": gc.SCALE_DIV, "cs_mode": gc.SCALE_MUL}, {"alpha": gc.ALPHA, "beta": gc.BETA}):
        truth, bound = gc.truth_and_bound(case, ops, dt, **kw)
        r = gc.assert_within(_cpu_result(case, ops, dt, **kw), truth, bound, f"{gc.case_id(case)} {kw}")
        assert 0.0 <= r <= 1.0
    assert (bound > 0).all()


@pytest.mark.parametrize("case", REPRESENTATIVE, ids=IDS)
def test_one_dropped_k_term_fails_the_bound(case):
    dt = torch.float64
    ops = gc.operands(case, dt)
    truth, bound = gc.truth_and_bound(case, ops, dt)
    got = _cpu_result(case, ops, dt)
    gc.assert_within(got, truth, bound)
    b, i, j, k = case.B - 1, case.M - 1, case.N // 2, case.K - 1
    got[b, i, j] -= gc.op(ops.A, case.tA)[b, i, k] * gc.op(ops.Bm, case.tB)[b, k, j]
    with pytest.raises(AssertionError, match=rf"element \({b}, {i}, {j}\)"):
        gc.assert_within(got, truth, bound)


@pytest.mark.parametrize("dt", gc.DTYPES)
@pytest.mark.parametrize("case", REPRESENTATIVE, ids=IDS)
def test_one_dropped_k_term_fails_the_exact_comparison(case, dt):
    ops = gc.int_operands(case, dt)
    for kw in ({}, {"rs_mode": gc.SCALE_DIV, "cs_mode": gc.SCALE_MUL}, {"alpha": gc.ALPHA, "beta": gc.BETA}):
        truth, _ = gc.truth_and_bound(case, ops, dt, **kw)
        got = _cpu_result(case, ops, dt, **kw)
        gc.assert_exact(got, truth)                      # the data is exact in dt: plain arithmetic reproduces the fp64 truth
    truth, _ = gc.truth_and_bound(case, ops, dt)
    got = _cpu_result(case, ops, dt)
    A, Bm = gc.op(ops.A, case.tA), gc.op(ops.Bm, case.tB)
    b, i, j = 0, case.M // 2, case.N - 1
    k = int((A[b, i, :] * Bm[b, :, j]).abs().argmax())   # a term that is not zero
    assert A[b, i, k] * Bm[b, k, j] != 0
    got[b, i, j] -= A[b, i, k] * Bm[b, k, j]
    with pytest.raises(AssertionError, match="1 of"):
        gc.assert_exact(got, truth)


@pytest.mark.parametrize("dt", gc.DTYPES)
@pytest.mark.parametrize("case", REPRESENTATIVE, ids=IDS)
def test_one_element_left_at_the_sentinel_fails(case, dt):
    for ops, check in ((gc.operands(case, dt), gc.assert_within), (gc.int_operands(case, dt), None)):
        truth, bound = gc.truth_and_bound(case, ops, dt)
        got = _cpu_result(case, ops, dt)
        got[case.B - 1, 0, case.N - 1] = gc.SENTINEL
        with pytest.raises(AssertionError):
            if check is None:
                gc.assert_exact(got, truth)
            else:
                check(got, truth, bound)
    got = _cpu_result(case, ops, dt)
    got[0, case.M - 1, 0] = float("nan")                 # what a read past an operand's extent returns
    with pytest.raises(AssertionError):
        gc.assert_within(got, truth, bound)


@pytest.mark.parametrize("dt", gc.DTYPES)
def test_a_write_outside_the_output_window_fails_the_guards(dt):
    M, N, B = 5, 7, 2
    p = gc.Padded((B, M, N), dt, N + 5, M * (N + 5) + 7, gc.SENTINEL)
    p.view().copy_(torch.randn(B, M, N).to(dt))
    gc.assert_guards(p, p.buf)
    assert torch.count_nonzero(p.buf == torch.tensor(gc.SENTINEL, dtype=dt)) == p.buf.numel() - B * M * N
    for flat in (p.start - 1,                            # before the first element
                 p.start + N,                            # the first padding column of row 0
                 p.start + M * p.ld,                     # between the items
                 p.start + p.stride + (M - 1) * p.ld + N,  # right after the last element
                 p.buf.numel() - 1):
        buf = p.buf.clone()
        buf[flat] = 0.0
        with pytest.raises(AssertionError, match="outside the output window"):
            gc.assert_guards(p, buf)
    buf = p.buf.clone()
    buf[p.start - 1] = -gc.SENTINEL                      # the bits are compared, not the magnitude
    with pytest.raises(AssertionError):
        gc.assert_guards(p, buf)


def test_integer_operands_stay_exact_in_fp32():
    assert len(gc.ALL_CASES) > 300
    for case in gc.ALL_CASES:
        assert 9 * case.K < 2 ** 24, case
    for case in REPRESENTATIVE + [gc.BIG_SPLIT_CASE, gc.sym_case(*gc.SYM_CASES[2])]:
        ops = gc.int_operands(case, torch.float32)
        for x in (ops.A, ops.Bm, ops.C):
            assert torch.equal(x, x.round()) and x.abs().max() <= 3
        for s in (ops.rs, ops.cs):
            assert torch.equal(torch.frexp(s)[0], torch.full_like(s, 0.5)) and 0.25 <= s.min() and s.max() <= 4


def test_threshold_scales_straddle_the_smallest_normal():
    for dt in gc.DTYPES:
        s = gc.threshold_scales(dt)
        tiny = torch.finfo(dt).tiny
        assert (s[:4].abs() < tiny).all() and (s[4:].abs() == tiny).all() and s[2] > 0 and s[3] > s[2] and torch.signbit(s[1])
        case = gc.Case(6, 3, 4, False, False, 1)
        ops = gc.operands(case, dt)
        ops = ops._replace(A=ops.A * 2.0 ** -8, rs=s[None, :].clone())   # (|P| < 1: the quotient by the smallest normal is finite)
        truth, bound = gc.truth_and_bound(case, ops, dt, rs_mode=gc.SCALE_DIV)
        assert (truth[0, :4] == 0).all() and (bound[0, :4] == 0).all() and torch.isfinite(truth).all() and (truth[0, 4:] != 0).all()

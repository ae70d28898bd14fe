"""The tests of the sweep-kernel tests (sweep_cases.py), without a GPU: on every graded case the GPU file uses, the faithful
algorithm emulated in the working precision with torch stays far inside the derived entry-wise bounds (they are reachable), and
the rewrites the bounds exist to refuse exceed them (they are not vacuous): the one-pass Gram matrix V1^T (M M^T) V1 in place of
the Gram matrix of the rotated rows, a projection whose U has two columns exchanged, and one that scales with another item's
sigma.  The mirrored split_range partitions every chunk exactly once.  Every ratio is printed (`pytest -s`)."""
import pytest
import torch

import sweep_cases as sc
from matrix_cases import assert_within

DT = pytest.mark.parametrize("dt", sc.DTYPES, ids=["f32", "f64"])
GRADED = pytest.mark.parametrize("case", sc.GRADED, ids=lambda c: "R{}-n{}-d{}".format(*c))


def what(kind, case, dt):
    return "{} R={} n={} decay={} {}".format(kind, *case, sc.dt_name(dt))


def test_graded_operands_are_what_the_docstring_says():
    for R, n, decay in sc.GRADED:
        for dt in sc.DTYPES:
            M, V1, V2, sigma, sigma1 = sc.graded_batch(R, n, decay, dt)
            assert M.shape == (3, R, n) and V1.shape == V2.shape == (3, R, R) and sigma.shape == sigma1.shape == (3, R)
            assert all(t.dtype == dt for t in (M, V1, V2, sigma, sigma1))
            s = torch.linalg.svdvals(M.double())
            for b, scale in enumerate(sc.ITEM_SCALES):
                want = scale * 2.0 ** (-decay * torch.arange(R, dtype=torch.float64))
                assert ((s[b] - want).abs() <= 1e-3 * want + 64 * sc.unit(dt) * want[0]).all()     # graded, and scaled
                assert float(want[-1]) ** 2 > 2.0 ** -100 * scale ** 2
                # sigma of pass 2: sorted, and the kept half (the projections' ro = R / 2) carries its small values to a relative error
                assert (sigma[b, :-1] >= sigma[b, 1:]).all() and float(sigma[b, R // 2 - 1]) > 0
                assert ((sigma[b].double() - want).abs() <= 1e-3 * want)[:R // 2].all()
            I = torch.eye(R, dtype=torch.float64)
            assert ((V1.double().transpose(1, 2) @ V1.double()) - I).abs().max() < 64 * sc.unit(dt)


@DT
@GRADED
def test_faithful_gram_is_within_the_bound_and_the_shortcut_is_not(case, dt):
    R, n, decay = case
    M, V1, _, _, _ = sc.graded_batch(R, n, decay, dt)
    parts = sc.pick_split(n, 3)
    G, bound = sc.gram_truth_and_bound(M, V1, dt, parts)
    assert_within(sc.emulate_gram(M, V1), G, bound, what("rotgram faithful", case, dt))
    faithful = sc.ratio(sc.emulate_gram(M, V1), G, bound)
    short = sc.emulate_shortcut(M, V1)
    per_item = [sc.ratio(short[b:b + 1], G[b:b + 1], bound[b:b + 1]) for b in range(3)]
    print("{}: faithful {:.4f}, shortcut per item {}".format(what("rotgram", case, dt), faithful, ["%.1f" % r for r in per_item]))
    assert faithful <= 1.0
    assert min(per_item) > 1.0, "not a graded case: the one-pass shortcut stays within the bound"
    G1, bound1 = sc.gram_truth_and_bound(M, None, dt, parts)
    assert_within(sc.emulate_gram(M), G1, bound1, what("rowgram faithful", case, dt))
    # the tall kernels: the same formulas on the transpose
    Gc, boundc = sc.colgram_truth_and_bound(M.transpose(1, 2), V1, dt, 1)
    assert torch.equal(Gc, sc.gram_truth_and_bound(M, V1, dt, 1)[0])
    Mt = M.transpose(1, 2).contiguous()
    W = Mt @ V1
    assert_within(W.transpose(1, 2) @ W, Gc, boundc, what("colgram faithful", case, dt))


@DT
@GRADED
@pytest.mark.parametrize("with_v1", [True, False], ids=["V1", "noV1"])
@pytest.mark.parametrize("scale", [1, 0], ids=["scaled", "plain"])
def test_faithful_project_is_within_the_bound_and_damage_is_not(case, dt, with_v1, scale):
    R, n, decay = case
    M, V1, V2, sigma, _ = sc.graded_batch(R, n, decay, dt)
    ro = max(R // 2, 2)
    if with_v1:
        v1, v2 = V1, V2
    else:   # U handed over ready: the rounded product
        v1, v2 = None, (V1.double() @ V2.double()).to(dt)
    right, rb, left, lb = sc.project_truth_and_bounds(M, v1, v2, sigma, ro, scale, dt)
    r, l = sc.emulate_project(M, v1, v2, sigma, ro, scale)
    tag = what("project{}{}".format(" V1" if with_v1 else "", " scaled" if scale else ""), case, dt)
    assert_within(r, right, rb, tag + " right")
    assert_within(l, left, lb, tag + " left")
    r, l = sc.emulate_project(M, v1, v2, sigma, ro, scale, swap=(0, 1))
    swapped = (sc.ratio(r, right, rb), sc.ratio(l, left, lb))
    print("{}: columns 0 and 1 of U exchanged: right {:.3g}, left {:.3g} of the bound".format(tag, *swapped))
    assert min(swapped) > 1.0
    if scale:
        r, l = sc.emulate_project(M, v1, v2, sigma, ro, scale, sigma_roll=1)
        rolled = (sc.ratio(r, right, rb), sc.ratio(l, left, lb))
        print("{}: sigma of the neighbouring item: right {:.3g}, left {:.3g} of the bound".format(tag, *rolled))
        assert min(rolled) > 1.0
    # the tall kernel's results are the transposes
    cl, clb, cr, crb = sc.colproject_truth_and_bounds(M.transpose(1, 2), v1, v2, sigma, ro, scale, dt)
    assert torch.equal(cl, right.transpose(1, 2)) and torch.equal(cr, left.transpose(1, 2))
    assert torch.equal(clb, rb.transpose(1, 2)) and torch.equal(crb, lb.transpose(1, 2))


@DT
def test_flags_change_the_truth_as_the_header_says(dt):
    """rows32: rows 32.. count as zero whatever they hold; flat: U = V1[:, :ro], scales from sigma1, V2 and sigma not looked at;
    a sigma below the smallest normal: exact zeros in right, bound 0."""
    M, V1, V2, sigma, sigma1 = (t.clone() for t in sc.random_batch(4, 37, 20, dt))
    f = torch.tensor([1, 0, 1, 0], dtype=torch.int32)
    Mn = M.clone()
    Mn[f.bool(), 32:] = float("nan")
    G, b = sc.gram_truth_and_bound(Mn, V1, dt, 1, rows32=f)
    M0 = M.clone()
    M0[f.bool(), 32:] = 0
    G0, b0 = sc.gram_truth_and_bound(M0, V1, dt, 1)
    assert torch.equal(G, G0) and torch.equal(b, b0) and torch.isfinite(G).all()
    W = V1[0, :32].double().T @ M[0, :32].double()
    assert (G[0] - W @ W.T).abs().max() <= 1e-12 * G[0].abs().max()
    V2n, sn = V2.clone(), sigma.clone()
    V2n[f.bool()] = float("nan")
    sn[f.bool()] = float("nan")
    ro = 5
    right, rb, left, lb = sc.project_truth_and_bounds(M, V1, V2n, sn, ro, 1, dt, flat=f, sigma1=sigma1)
    assert all(torch.isfinite(t).all() for t in (right, rb, left, lb))
    U = V1[0, :, :ro].double()
    assert torch.equal(left[0], U * sigma1[0, :ro].double()) and torch.equal(right[0], (U.T @ M[0].double()) * (1.0 / sigma1[0, :ro].double())[:, None])
    assert torch.equal(lb[0], sc.SPARE * sc.unit(dt) * left[0].abs() + 37 * 20 * sc.tiny(dt))
    same = sc.project_truth_and_bounds(M, None, V2, sigma, ro, 1, dt, flat=f, sigma1=sigma1)     # without V1 the flags are ignored
    plain = sc.project_truth_and_bounds(M, None, V2, sigma, ro, 1, dt)
    assert all(torch.equal(a, c) for a, c in zip(same, plain))
    sz = sigma.clone()
    sz[:, 1] = sc.tiny(dt) / 4
    right, rb, left, lb = sc.project_truth_and_bounds(M, V1, V2, sz, ro, 1, dt)
    assert not right[:, 1].any() and not rb[:, 1].any() and bool((rb[:, 0] > 0).all()) and bool(left[:, :, 1].any())


def test_split_range_partitions_every_chunk_once():
    pairs = {((sc.NPARTS_N + 15) // 16, q) for q in sc.NPARTS}
    pairs |= {((n + 31) // 32, parts) for n, parts in sc.PROJECT_SPLIT_N} | {((rows + 15) // 16, parts) for rows, parts in sc.COL_SPLIT_ROWS}
    pairs |= {((n + 15) // 16, sc.pick_split(n, 3)) for _, n, _ in sc.GRADED} | {(1, 1), (5, 1), (63, 64), (4375, 64)}
    for chunks, nparts in sorted(pairs):
        seen = [0] * chunks
        last = 0
        for q in range(nparts):
            c0, c1 = sc.split_range(chunks, nparts, q)
            assert c0 == q * -(-chunks // nparts) and c1 <= chunks
            if c1 > c0:
                assert c0 == last
                last = c1
            for c in range(c0, c1):
                seen[c] += 1
        assert seen == [1] * chunks and last == chunks, (chunks, nparts, seen)
    # parts without a chunk exist in the caller-chosen cases, and their column range is empty
    assert sc.split_range(7, 9, 7) == (7, 7) and sc.part_columns(100, 9, 8) == (100, 100)
    assert [sc.part_columns(100, 3, q) for q in range(3)] == [(0, 48), (48, 96), (96, 100)]


def test_mirrored_part_counts():
    """pick_split / col_split as the issue's edge list needs them: ragged last shares, `left` / `right` written by part 0 alone."""
    assert [sc.pick_split(n, 2) for n, _ in sc.PROJECT_SPLIT_N] == [p for _, p in sc.PROJECT_SPLIT_N]
    assert [sc.col_split(r, 2) for r, _ in sc.COL_SPLIT_ROWS] == [p for _, p in sc.COL_SPLIT_ROWS]
    assert sc.pick_split(1000, 5) == 4 and sc.pick_split(100, 3) == 1 and sc.col_split(65, 5) == 1 and sc.col_split(1000, 5) == 3
    assert sc.pick_split(2048, 256) == 8 and sc.pick_split(208, 256) == 1


def test_threshold_rules():
    s = torch.tensor([[1.0, 0.5, 0.125], [1.0, 0.5, 0.1249], [0.0, 0.0, 0.0]], dtype=torch.float64)
    assert sc.spectrum_flat_rule(s, 3, 0.125).tolist() == [1, 0, 0] and sc.spectrum_flat_rule(s, 1, 0.125).tolist() == [1, 1, 0]
    Rm = torch.zeros(2, 64, 3, dtype=torch.float64)
    Rm[:, 0, 0] = 1.0
    eps = torch.finfo(torch.float32).eps
    Rm[0, 40, 1] = 8 * eps * 0.999
    Rm[1, 40, 1] = 8 * eps * 1.001
    assert sc.carry_rows32_rule(Rm, 8, torch.float32).tolist() == [1, 0]

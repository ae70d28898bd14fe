"""The kernels of csrc/ttr_index.hip behind ttr_gather_chain on the sorted path and at their size edges, each against the plain
fp64 chain of tests/indexing_cases.py (whose references tests/test_indexing_cases_host.py checks against brute-force loops).
Routing cases use integer cores (entries in {-2 .. 2}, every partial sum far below 2^24): the device result is exact in fp32 and
fp64, so they assert torch.equal against the reference, and bitwise equality of the sorted and the direct path.  Float cases use
the derived bound |out - ref| <= 2 (sum over the multiplied modes of (r_n + 2)) u scale, scale the chain over |G|.

Which branch each group of cases reaches, per kernel:
- validate_kernel: P on both sides of its 256-thread workgroups and one point (test_point_counts_and_default_switch); a bad entry
  in the first and the last lane of the launch, int32 and int64, in every mode (test_out_of_range_sorted_path).
- histogram_kernel / scatter_kernel: the LDS branch at I = 1023, 1024 and the global-atomic branch (!lds) from I = 1025 on
  (test_bins_and_scan_chunks), most bins hit (P = 5000) and most bins empty (P = 300), all points in two bins (contended global
  atomics), several workgroups and a ragged last one; both branches in one chain whose cnt / cursor are reused from mode to mode
  (test_mode_sizes_change_along_the_chain); the return on a set flag (test_out_of_range_sorted_path: a scatter that ran on a bad
  column would leave perm entries unwritten for the step to read).
- scan_kernel: one, two and three chunks of 1024 bins with full and ragged last chunks, the carry0 / carry1 hand-over, a first chunk
  of zeros (carry starts at 0), only the first and the last bin (test_bins_and_scan_chunks); toff[I] at a position that moves from
  mode to mode, over stale entries of a larger earlier call (test_mode_sizes_change_along_the_chain); ra in the tile count
  (test_leading_rank_*, test_group_sizes_on_tile_edges).
- gather_kernel: one-mode chains as a pure gather, P ra rn past 65536 * 256 (the grid-stride loop's second trip), strided cores and
  `out` (test_one_mode_*, test_output_and_core_strides).
- step_kernel, direct: tpp = 1 (ra <= 64) and tpp = 2, 3, 8 with a ragged last tile per point (test_leading_rank_*); grid z = 65535
  (test_batch_limit).
- step_kernel, sorted: tiles that straddle points (ra = 3, 63, 65, 130), rend clipped at the end of a group, groups that end on
  a tile boundary, empty groups between full ones in the tile search (test_group_sizes_on_tile_edges, test_leading_rank_*); k
  chunks of 32 and column tiles of 64 crossed at ra > 64 (test_leading_rank_gaussian); any strides of `out` and of the cores
  (test_output_and_core_strides); the return on a set flag (test_out_of_range_sorted_path).
- the entry: index columns as int32 / int64 with negative values, columns of a [P, N] matrix, a stride-0 column, mixed dtypes
  (test_index_column_forms); P = 0 (test_no_points*); the default switch at P = 1024 / 1025; ranks 512 / 513, batch 65535 / 65536, a workspace one
  byte short (test_limits_rank, test_batch_limit, test_workspace_one_byte_short); Tensor.__getitem__ with a bond rank of 65 and a mode of 1500 (test_public_api).

No case hands the kernel an index that it could turn into an access out of bounds if the check failed to stop it: the bad values are
I and -I - 1 only, against cores allocated with a spare slice on each side of the I axis and passed as the slice [1, I + 1) of
that allocation, so the slice a wrongly accepted I or -1 would address is allocated memory; histogram, scatter and the tile
search skip an out-of-range value by themselves (idx_value gives -1)."""
from ctypes import c_int64, c_void_p

import pytest
import torch

import indexing_cases as ic
import tntorch_amd as tn
from tntorch_amd import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.float64]
PATHS = (ic.SORTED, ic.DIRECT)
SENTINEL = -7.5


def on_dev(cores, dtype):
    return [c.to(DEV, dtype) for c in cores]


def run(cores, cols, dm, out=None):
    """gather_chain into ``out``, or into a fresh tensor filled with NaN: an element the kernels leave unwritten shows."""
    if out is None:
        out = torch.full((cores[0].shape[0], cores[0].shape[1], cols[0].shape[0], cores[-1].shape[3]), float("nan"),
                         dtype=cores[0].dtype, device=DEV)
    res = _hip.gather_chain(cores, [c.to(DEV) for c in cols], out=out, direct_max_points=dm)
    assert res is out
    return out


def assert_exact(out, ref, what=None):
    got = out.double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.equal(got, ref), (what, int((got != ref).sum()), float((got - ref).abs().max()))


def both_paths_exact(cores, cols, ref, what=None):
    """Each forced path equals the reference, and the two outputs are equal bit for bit; returns the sorted one."""
    a, b = run(cores, cols, ic.SORTED), run(cores, cols, ic.DIRECT)
    assert_exact(a, ref, (what, "sorted"))
    assert_exact(b, ref, (what, "direct"))
    assert torch.equal(a, b), what
    return a


def assert_within_bound(out, ref, scale, ranks, dtype, what=None):
    err, bound = (out.double().cpu() - ref).abs(), ic.error_bound(ranks, dtype, scale)
    print(what, dtype, "max err / bound", float((err / (bound + 1e-300)).max()))
    assert bool((err <= bound).all()), (what, float((err / (bound + 1e-300)).max()))


def raw_args(cores, cols):
    n = len(cores)
    ranks = (c_int64 * (n + 1))(*([int(c.shape[1]) for c in cores] + [int(cores[-1].shape[3])]))
    sizes = (c_int64 * n)(*[int(c.shape[2]) for c in cores])
    return n, ranks, sizes


def workspace_bytes(cores, cols):
    n, ranks, sizes = raw_args(cores, cols)
    return int(_hip.lib().ttr_gather_chain_workspace_bytes(_hip.dtype_code(cores[0].dtype), n, ranks, sizes, cols[0].shape[0], cores[0].shape[0]))


def raw_chain(cores, cols, out, ws, ws_bytes, dm, flag):
    """ttr_gather_chain through the C ABI with the caller's workspace and flag word (int64 device columns)."""
    n, ranks, sizes = raw_args(cores, cols)
    assert all(c.dtype == torch.int64 and c.is_cuda for c in cols) and ws.numel() >= ws_bytes
    ptrs = (c_void_p * n)(*[c.data_ptr() for c in cores])
    strides = (c_int64 * (4 * n))(*[int(s) for c in cores for s in c.stride()])
    iptrs = (c_void_p * n)(*[i.data_ptr() for i in cols])
    istr = (c_int64 * n)(*[int(i.stride(0)) for i in cols])
    _hip._call("ttr_gather_chain", _hip.dtype_code(cores[0].dtype), n, cores[0].shape[0], cols[0].shape[0], ranks, sizes, ptrs, strides,
               1, iptrs, istr, out.data_ptr(), *[int(s) for s in out.stride()], int(dm), flag.data_ptr(), ws.data_ptr(), int(ws_bytes))


# ---------------------------------------------------------------------------------------------------- 1. bins and scan chunks
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("I", ic.BINS_I)
def test_bins_and_scan_chunks(I, dtype):
    name = "bins_{}".format(I)
    cores64 = ic.case_cores(name)
    cores = on_dev(cores64, dtype)
    sizes = ic.INT_CASES[name][1]
    for P in ic.BINS_P:
        cols = ic.random_cols(sizes, P, 100 + P)
        hit = int(torch.unique(ic.wrapped(cols[1], I)).numel())
        assert hit > 0.75 * I if P == 5000 else hit < 0.3 * I  # most values hit / most groups empty
        assert_exact(run(cores, cols, ic.SORTED), ic.cached_reference((name, P), cores64, cols), (I, P))


@pytest.mark.parametrize("dtype", DTYPES)
def test_scan_first_chunk_empty_and_end_bins(dtype):
    """Only values >= 1024 at I = 3000: the first scan chunk is all zeros and the carry starts at 0.  Only the values 0 and
    I - 1 at I = 2049: the first bin of the first chunk and the only bin of the third, 2500 points on two global counters."""
    P = 5000
    g = torch.Generator().manual_seed(41)
    for name, draw in (("bins_3000", lambda I: torch.randint(ic.SCAN_CHUNK, I, (P,), generator=g)),
                       ("bins_2049", lambda I: torch.randint(0, 2, (P,), generator=g) * (I - 1))):
        cores64 = ic.case_cores(name)
        sizes = ic.INT_CASES[name][1]
        cols = [torch.randint(0, sizes[0], (P,), generator=g), draw(sizes[1]), draw(sizes[2])]
        if name == "bins_3000":
            assert int(cols[1].min()) >= ic.SCAN_CHUNK and int(cols[2].min()) >= ic.SCAN_CHUNK
        else:
            assert sorted(torch.unique(cols[1]).tolist()) == [0, sizes[1] - 1]
        assert_exact(run(on_dev(cores64, dtype), cols, ic.SORTED), ic.cached_reference((name, "extra"), cores64, cols), name)


# ------------------------------------------------------------------------------------- 2. mode sizes that change along the chain
@pytest.mark.parametrize("dtype", DTYPES)
def test_mode_sizes_change_along_the_chain(dtype):
    P = ic.CHANGING_P
    small64, large64 = ic.case_cores("changing"), ic.case_cores("changing_larger")
    small, large = on_dev(small64, dtype), on_dev(large64, dtype)
    cols_s, cols_l = ic.random_cols(ic.CHANGING_SIZES, P, 51), ic.random_cols(ic.CHANGING_LARGER, P, 52)
    ref_s, ref_l = ic.cached_reference("changing", small64, cols_s), ic.cached_reference("changing_larger", large64, cols_l)
    both_paths_exact(small, cols_s, ref_s, "alone")
    # right after a call with larger sizes, through the wrapper (whose scratch comes from the caching allocator) ...
    assert_exact(run(large, cols_l, ic.SORTED), ref_l, "larger")
    both_paths_exact(small, cols_s, ref_s, "after larger")
    # ... and through the C ABI on one workspace of the test's own: cnt / off / toff hold the larger call's entries above I
    dl, ds = [c.to(DEV) for c in cols_l], [c.to(DEV) for c in cols_s]
    nbytes = workspace_bytes(large, dl)
    assert nbytes >= workspace_bytes(small, ds)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    out_l, out_s = torch.empty(ref_l.shape, dtype=dtype, device=DEV), torch.empty(ref_s.shape, dtype=dtype, device=DEV)
    raw_chain(large, dl, out_l, ws, nbytes, ic.SORTED, flag)
    raw_chain(small, ds, out_s, ws, nbytes, ic.SORTED, flag)
    assert int(flag) == 0
    assert_exact(out_l, ref_l, "raw larger")
    assert_exact(out_s, ref_s, "raw after larger")


# ------------------------------------------------------------------------------------------------------------ 3. leading rank
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ra", ic.LEAD_RA)
def test_leading_rank_integer(ra, dtype):
    name = "lead_{}".format(ra)
    cores64 = ic.case_cores(name)
    assert not torch.equal(cores64[1][0], cores64[1][1])  # different cores per batch item
    cols = ic.random_cols([ic.LEAD_I] * 3, ic.LEAD_P, 60 + ra)
    out = both_paths_exact(on_dev(cores64, dtype), cols, ic.cached_reference(name, cores64, cols), ra)
    assert out.shape == (ic.LEAD_B, ra, ic.LEAD_P, 2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ra", ic.LEAD_RA)
def test_leading_rank_gaussian(ra, dtype):
    ranks = ic.lead_ranks(ra, gauss=True)
    cores = ic.gauss_cores(ranks, [ic.LEAD_I] * 3, ic.LEAD_B, 70 + ra, dtype)
    cols = ic.random_cols([ic.LEAD_I] * 3, ic.LEAD_P, 80 + ra)
    ref, scale = ic.chain_reference(cores, cols)
    dc = on_dev(cores, dtype)
    a, b = run(dc, cols, ic.SORTED), run(dc, cols, ic.DIRECT)
    assert_within_bound(a, ref, scale, ranks, dtype, ("sorted", ra))
    assert_within_bound(b, ref, scale, ranks, dtype, ("direct", ra))
    assert torch.equal(a, b), ra


# ------------------------------------------------------------------------------------------------- 4. group sizes on tile edges
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ra", list(ic.TILE_EDGE_COUNTS))
def test_group_sizes_on_tile_edges(ra, dtype):
    name, counts = "tile_edges_{}".format(ra), ic.TILE_EDGE_COUNTS[ra]
    cores64 = ic.case_cores(name)
    P = sum(counts)
    cols = [ic.random_cols([4], P, 90 + ra)[0], ic.counts_column(counts, 91 + ra), ic.counts_column(counts, 92 + ra)]
    assert not torch.equal(cols[1], cols[2])
    ref = ic.cached_reference(name, cores64, cols)
    assert_exact(run(on_dev(cores64, dtype), cols, ic.SORTED), ref, ra)


# ---------------------------------------------------------------------------------------- 5. point counts and the default switch
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", ic.SWITCH_P)
def test_point_counts_and_default_switch(P, dtype):
    cores64 = ic.case_cores("switch")
    cores = on_dev(cores64, dtype)
    cols = ic.random_cols(ic.SWITCH_SIZES, P, 200 + P)
    ref = ic.cached_reference(("switch", P), cores64, cols)
    forced = both_paths_exact(cores, cols, ref, P)
    out = run(cores, cols, ic.DEFAULT)
    assert_exact(out, ref, (P, "default"))
    assert torch.equal(out, forced), P


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dm", (ic.DEFAULT,) + PATHS)
def test_no_points(dm, dtype):
    cores = on_dev(ic.case_cores("switch"), dtype)
    for n in (1, 3):
        cols = [torch.empty(0, dtype=torch.int64, device=DEV) for _ in range(n)]
        out = _hip.gather_chain(cores[:n], cols, direct_max_points=dm)
        assert out.shape == (2, 2, 0, cores[n - 1].shape[3]) and out.dtype == dtype and out.is_cuda


def test_no_points_public_api():
    """t[idx] with an empty [0, N] index matrix on the device, as on the CPU: a [1, 0, 1] core."""
    cores = [c[0] for c in ic.gauss_cores([1, 3, 4, 1], [5, 6, 7], 1, 230, torch.float32)]
    t, h = tn.Tensor([c.to(DEV) for c in cores]), tn.Tensor(cores)
    got, want = t[torch.empty((0, 3), dtype=torch.int64, device=DEV)], h[torch.empty((0, 3), dtype=torch.int64)]
    assert [tuple(c.shape) for c in got.cores] == [tuple(c.shape) for c in want.cores] == [(1, 0, 1)] and got.cores[0].is_cuda


# -------------------------------------------------------------------------------------------- 6. index columns in their forms
def index_forms():
    """name -> the columns of the form, on the CPU; every form holds negative entries."""
    P, sizes = ic.FORMS_P, ic.FORMS_SIZES
    base = ic.random_cols(sizes, P, 300)
    assert all(bool((c < 0).any()) and bool((c >= 0).any()) for c in base)
    forms = {"int64": base, "int32": [c.to(torch.int32) for c in base]}
    M = torch.stack(base, 1)
    forms["matrix_int64"] = [M[:, n] for n in range(3)]
    M32 = M.to(torch.int32)
    forms["matrix_int32"] = [M32[:, n] for n in range(3)]
    for n, v in ((0, -2), (1, 3), (2, -1)):  # one element expanded to P entries: every point in one group
        cols = list(base)
        cols[n] = torch.tensor([v]).expand(P)
        forms["stride0_mode{}".format(n)] = cols
    forms["mixed"] = [base[0], base[1].to(torch.int32), base[2]]
    return forms


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["int64", "int32", "matrix_int64", "matrix_int32", "stride0_mode0", "stride0_mode1", "stride0_mode2",
                                  "mixed"])
def test_index_column_forms(form, dtype):
    cols = index_forms()[form]
    cores64 = ic.case_cores("forms")
    dcols = [torch.stack(cols, 1).to(DEV)[:, n] for n in range(3)] if form.startswith("matrix") else \
        [c[:1].to(DEV).expand(ic.FORMS_P) if c.stride(0) == 0 else c.to(DEV) for c in cols]
    if form.startswith("matrix"):
        assert all(c.stride(0) == 3 for c in dcols)
    if form.startswith("stride0"):
        assert sum(c.stride(0) == 0 for c in dcols) == 1
    if form == "mixed":
        assert {c.dtype for c in dcols} == {torch.int32, torch.int64}
    ref = ic.cached_reference(("forms", form.replace("int32", "int64").replace("mixed", "int64")), cores64, cols)
    cores = on_dev(cores64, dtype)
    a, b = run(cores, dcols, ic.SORTED), run(cores, dcols, ic.DIRECT)
    assert_exact(a, ref, (form, "sorted"))
    assert_exact(b, ref, (form, "direct"))
    assert torch.equal(a, b), form


# ------------------------------------------------------------------------------------------------ 7. output and core strides
def strided_cores(cores, kind):
    """The same values as a slice of a larger tensor (every stride above the contiguous one) or with the I stride equal to 1."""
    res = []
    for c in cores:
        B, r, I, rn = c.shape
        if kind == "slice":
            big = torch.full((B + 1, r + 2, I + 3, rn + 1), SENTINEL, dtype=c.dtype, device=c.device)
            v = big[1:, 1:r + 1, 2:I + 2, :rn]
            v.copy_(c)
            assert v.stride() == ((r + 2) * (I + 3) * (rn + 1), (I + 3) * (rn + 1), rn + 1, 1)
        else:
            v = c.transpose(2, 3).contiguous().transpose(2, 3)
            assert v.stride(2) == 1 and v.shape == c.shape
        res.append(v)
    return res


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("core_kind", ["slice", "istride1"])
@pytest.mark.parametrize("name", ["strides_1", "strides_3"])
def test_output_and_core_strides(name, core_kind, dtype):
    P = 1500
    ranks, sizes, B = ic.INT_CASES[name]
    cores64 = ic.case_cores(name)
    cols = ic.random_cols(sizes, P, 400)
    ref = ic.cached_reference(name, cores64, cols)
    cores = strided_cores(on_dev(cores64, dtype), core_kind)
    for dm in PATHS:
        buf = torch.full((B, P, ranks[0], ranks[-1]), SENTINEL, dtype=dtype, device=DEV)
        out = buf.permute(0, 2, 1, 3)  # [B, r_0, P, r_N] over a [B, P, r_0, r_N] buffer
        run(cores, cols, dm, out=out)
        assert_exact(out, ref, (name, core_kind, dm, "permuted"))
        pad = torch.full((B + 2, ranks[0] + 2, P + 3, ranks[-1] + 2), SENTINEL, dtype=dtype, device=DEV)
        out = pad[1:-1, 1:-1, 2:-1, 1:-1]
        run(cores, cols, dm, out=out)
        assert_exact(out, ref, (name, core_kind, dm, "padded"))
        inside = torch.zeros(pad.shape, dtype=torch.bool, device=DEV)
        inside[1:-1, 1:-1, 2:-1, 1:-1] = True
        assert bool((pad[~inside] == SENTINEL).all()), (name, core_kind, dm)  # the padding stays untouched


# ------------------------------------------------------------------------------------------------------- 8. one-mode chains
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P,ra,rn,I,B", ic.ONE_MODE)
def test_one_mode_is_a_gather(P, ra, rn, I, B, dtype):
    g = torch.Generator().manual_seed(P + ra)
    G = torch.randn(B, ra, I, rn, generator=g, dtype=torch.float64).to(dtype)
    idx = torch.randint(-I, I, (P,), generator=g)
    want = G.index_select(2, ic.wrapped(idx, I))
    for dm in (ic.DEFAULT,) + PATHS:
        out = run([G.to(DEV)], [idx], dm)
        assert torch.equal(out.cpu(), want), (P, ra, rn, I, B, dm)


def test_one_mode_grid_stride_loop():
    P, ra, rn, I, B = ic.ONE_MODE_BIG
    assert P * ra * rn > ic.GATHER_GRID * ic.THREADS
    g = torch.Generator().manual_seed(5)
    G = torch.randn(B, ra, I, rn, generator=g)
    idx = torch.randint(-I, I, (P,), generator=g)
    out = run([G.to(DEV)], [idx], ic.DEFAULT)
    assert torch.equal(out.cpu(), G.index_select(2, ic.wrapped(idx, I)))


# -------------------------------------------------------------------------------------------- 9. out of range, sorted path
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dm,P", [(ic.SORTED, 1000), (ic.DEFAULT, 3000)])
@pytest.mark.parametrize("I", ic.OOB_I)
def test_out_of_range_sorted_path(I, dm, P, dtype):
    """One bad entry (I or -I - 1) in one mode at one point: IndexError, `out` untouched, and the next call is exact."""
    assert P > ic.DIRECT_MAX or dm == ic.SORTED
    alloc64 = ic.case_cores("oob_{}".format(I))
    alloc = on_dev(alloc64, dtype)
    cores = [c[:, :, 1:I + 1, :] for c in alloc]  # a spare slice on each side of the I axis
    assert all(c.shape[2] == I and c.storage_offset() > 0 for c in cores)
    good = ic.random_cols([I] * 3, P, 500 + I)
    ref = ic.cached_reference(("oob", I, P), [c[:, :, 1:I + 1, :] for c in alloc64], good)
    dgood = [c.to(DEV) for c in good]
    dgood32 = [c.to(torch.int32) for c in dgood]
    for bad, idt in ((I, torch.int64), (-I - 1, torch.int64), (-I - 1, torch.int32), (I, torch.int32)):
        for mode in (0, 1, 2):
            for point in (0, P // 2, P - 1):
                cols = [c.clone() for c in (dgood if idt == torch.int64 else dgood32)]
                cols[mode][point] = bad
                out = torch.full(ref.shape, SENTINEL, dtype=dtype, device=DEV)
                with pytest.raises(IndexError):
                    _hip.gather_chain(cores, cols, out=out, direct_max_points=dm)
                assert bool((out == SENTINEL).all()), (bad, idt, mode, point)
                assert_exact(run(cores, dgood, dm), ref, ("after", bad, idt, mode, point))


# -------------------------------------------------------------------------------------------------------------- 10. limits
@pytest.mark.parametrize("where", [0, 1, 2])
def test_limits_rank(where):
    ranks = [2, 2, 2]
    ranks[where] = ic.MAX_RANK + 1
    cols = [torch.zeros(5, dtype=torch.int64, device=DEV) for _ in range(2)]
    cores = [torch.zeros(1, ranks[n], 2, ranks[n + 1], device=DEV) for n in range(2)]
    with pytest.raises(NotImplementedError, match="above 512"):
        _hip.gather_chain(cores, cols)
    ranks[where] = ic.MAX_RANK  # and the limit itself works
    cores64 = [torch.ones(1, ranks[n], 2, ranks[n + 1], dtype=torch.float64) for n in range(2)]
    out = run(on_dev(cores64, torch.float32), cols, ic.SORTED)
    assert_exact(out, ic.chain_reference(cores64, cols)[0], where)


@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_limit(dtype):
    with pytest.raises(NotImplementedError, match="above 65535"):
        _hip.gather_chain([torch.zeros(ic.MAX_BATCH + 1, 1, 1, 1, dtype=dtype, device=DEV)] * 2,
                          [torch.zeros(3, dtype=torch.int64, device=DEV)] * 2)
    cores64 = ic.case_cores("batch_limit")
    assert cores64[0].shape == (ic.MAX_BATCH, 1, 1, 1)
    cols = [torch.tensor([0, -1, 0]), torch.tensor([-1, 0, 0])]
    both_paths_exact(on_dev(cores64, dtype), cols, ic.cached_reference("batch_limit", cores64, cols), "batch")


@pytest.mark.parametrize("dtype", DTYPES)
def test_workspace_one_byte_short(dtype):
    cores64 = ic.case_cores("workspace")
    cores = on_dev(cores64, dtype)
    cols = [c.to(DEV) for c in ic.random_cols(ic.INT_CASES["workspace"][1], 2000, 600)]
    ref = ic.cached_reference("workspace", cores64, cols)
    nbytes = workspace_bytes(cores, cols)
    assert nbytes > 0
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    out = torch.full(ref.shape, SENTINEL, dtype=dtype, device=DEV)
    flag = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match=r"ttr_gather_chain failed \(-4\).*workspace"):  # TTR_E_WORKSPACE
        raw_chain(cores, cols, out, ws, nbytes - 1, ic.SORTED, flag)
    assert bool((out == SENTINEL).all()) and int(flag) == 5 and int(ws.max()) == 0
    raw_chain(cores, cols, out, ws, nbytes, ic.SORTED, flag)  # the reported size is enough
    assert int(flag) == 0
    assert_exact(out, ref, "exact size")


# ---------------------------------------------------------------------------------------------------------- 11. public API
@pytest.mark.parametrize("dtype", DTYPES)
def test_public_api(dtype):
    """t[:, ia, ib, :] (a chain with r_a = 65 whose sorted mode has I = 1500) and t[ia, ib, ic, :] on a device tensor against the same
    key on an fp64 CPU copy, within the derived bound of the chain the key produces; the cores the key only slices are equal.
    t[ia, ib, :, ic] is no chain: index arrays must be contiguous, as in the reference, so the device tensor and the CPU copy both
    refuse it with the same IndexError."""
    shape, ranks, P = ic.API_SHAPE, ic.API_RANKS, ic.API_P
    g = torch.Generator().manual_seed(700)
    c64 = [(torch.randn(ranks[n], shape[n], ranks[n + 1], generator=g, dtype=torch.float64) / ranks[n] ** 0.5).to(dtype).double()
           for n in range(4)]
    t, h = tn.Tensor([c.to(DEV, dtype) for c in c64]), tn.Tensor(c64)
    i0, ia, ib = ic.random_cols(shape[:3], P, 701)
    d0, da, db = i0.to(DEV), ia.to(DEV), ib.to(DEV)

    def check(got, want, block, cols, at):
        assert [tuple(c.shape) for c in got.cores] == [tuple(c.shape) for c in want.cores]
        ref, scale = ic.chain_reference([c64[n][None] for n in block], cols)
        assert float((want.cores[at] - ref[0]).abs().max()) <= 1e-13 * float(scale.max())  # the CPU copy is this chain
        chain_ranks = [ranks[block[0]]] + [ranks[n + 1] for n in block]
        for k, (a, b) in enumerate(zip(got.cores, want.cores)):
            assert a.is_cuda and a.dtype == dtype
            if k == at:
                assert_within_bound(a, b, scale[0], chain_ranks, dtype, ("api", block))
            else:
                assert torch.equal(a.double().cpu(), b), k

    check(t[:, da, db, :], h[:, ia, ib, :], [1, 2], [ia, ib], 1)
    check(t[d0, da, db, :], h[i0, ia, ib, :], [0, 1, 2], [i0, ia, ib], 0)
    i3 = ic.random_cols(shape[3:], P, 702)[0]
    for x, key in ((t, (d0, da, slice(None), i3.to(DEV))), (h, (i0, ia, slice(None), i3))):
        with pytest.raises(IndexError, match="contiguously"):
            x[key]

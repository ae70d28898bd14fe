"""ttr_maxvol, ttr_gather_step and device tn.cross at their edges, against plain fp64 references on the CPU:
- maxvol on exactly tied inputs (tests/golden/maxvol_ties_f64.npz), at r = 1 .. 128 and N from r + 1 to past the 256 argmax
  partials, a mixed batch, the tol / max_iters clamps, batch strides above N * r through the C ABI, and a zero column.  Exact rows
  and swap counts are asserted where every pivot decision of the reference (test_maxvol_host.ref_maxvol) either is an exact tie
  or has a relative gap of at least 1e-6 (fp64) / 1e-3 (fp32); the properties of a maximal-volume set are asserted everywhere;
- the gather step over its tile and chunk boundaries, strided and int32 inputs, and out-of-range entries;
- device cross: the first core holds the exact fibres and every later core interpolates (C[index] = I), so t at the points of
  the final right sets equals f there; the rank limit of 128 is raised before any work."""
import ctypes

import numpy as np
import pytest
import torch

import tntorch_amd as tn
from tntorch_amd import _hip
from test_maxvol_host import load_ties, ref_maxvol

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAP = {torch.float64: 1e-6, torch.float32: 1e-3}
EPS = {torch.float64: 2.0 ** -52, torch.float32: 2.0 ** -23}


def run_maxvol(A, tol=1.05, max_iters=100):
    """ttr_maxvol on a host [B, N, r] or [N, r] tensor -> (index, C, status) on the host."""
    A3 = A if A.dim() == 3 else A[None]
    status = torch.full((A3.shape[0], 2), -7, dtype=torch.int32, device=DEV)
    index, C = _hip.maxvol(A3.to(DEV), tol, max_iters, status=status)
    return index.cpu(), C.cpu(), status.cpu()


def host_ref(A, **kw):
    """The test reference on exactly the values the kernel sees (fp32 input rounded first)."""
    return ref_maxvol(A.double().numpy(), **kw)


def gaps_hold(res, dtype):
    return res.min_gap() >= GAP[dtype]


def check_properties(A, index, C, tol, dtype, name=""):
    """A maximal-volume set of rows: distinct, in range, |C| <= tol, C[index] = I, |det A[index]| at least the host mirror's."""
    N, r = A.shape
    small = 1e-3 if dtype == torch.float32 else 1e-8
    assert len(set(index.tolist())) == r and int(index.min()) >= 0 and int(index.max()) < N, name
    assert float(C.abs().max()) <= max(tol, 1.0) * (1 + small), (name, float(C.abs().max()))
    np.testing.assert_allclose(C[index].double().numpy(), np.eye(r), atol=small, err_msg=name)
    A64 = A.double()
    ih, _ = tn.maxvol(A64, tol=tol)
    ld_dev = torch.linalg.slogdet(A64[index])[1].item()
    ld_host = torch.linalg.slogdet(A64[ih])[1].item()
    assert ld_dev >= ld_host - 1e-3, (name, ld_dev, ld_host)


# ------------------------------------------------------------------------------------------------------------ maxvol: ties
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_maxvol_ties(dtype):
    """getrf's first-position rule (in one block, across blocks, across the 256 partials) and the column-first swap key."""
    for name, (A, it, tied, want) in load_ties().items():
        A = torch.as_tensor(A).to(dtype)
        res = host_ref(A, max_iters=it)
        assert res.decision(*tied).tied, name
        assert gaps_hold(res, dtype), (name, res.min_gap())
        np.testing.assert_array_equal(res.index, want, err_msg=name)
        index, C, status = run_maxvol(A, max_iters=it)
        np.testing.assert_array_equal(index[0].numpy(), want, err_msg=name)
        assert status[0].tolist() == [1, res.swaps], (name, status[0].tolist(), res.swaps)
        if tied[0] == "swap":  # the tied swap alone: which slot of index it fills shows the column order of the key
            res1 = host_ref(A, max_iters=1)
            assert res1.decision(*tied).tied and gaps_hold(res1, dtype), name
            index, C, status = run_maxvol(A, max_iters=1)
            np.testing.assert_array_equal(index[0].numpy(), res1.index, err_msg=name)
            assert status[0].tolist() == [1, 1], name


# ------------------------------------------------------------------------------------------------------------ maxvol: sizes
SHAPES = sorted({(N, r) for r in (1, 2, 63, 64, 65, 127, 128) for N in (r + 1, 15, 16, 17, 4096, 4097, 4112) if N > r})


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_maxvol_shapes(dtype):
    """Every (N, r) of SHAPES: exact rows and swap count where the reference's gaps hold, the properties everywhere.  fp64
    r = 128 uses 128 KB of dynamic LDS in the inverse."""
    exact = 0
    for N, r in SHAPES:
        g = torch.Generator().manual_seed(1000 * r + N)
        A = torch.randn(N, r, generator=g, dtype=torch.float64).to(dtype)
        index, C, status = run_maxvol(A)
        index, C = index[0], C[0]
        assert int(status[0, 0]) == 1 and 0 <= int(status[0, 1]) <= 100, (N, r)
        check_properties(A, index, C, 1.05, dtype, (N, r))
        res = host_ref(A)
        if gaps_hold(res, dtype):
            np.testing.assert_array_equal(index.numpy(), res.index, err_msg=str((N, r)))
            assert int(status[0, 1]) == res.swaps, (N, r)
            exact += 1
    # fp64: every seed is comparable exactly; fp32: a third of these seeds have a decision within 1e-3
    assert exact >= (len(SHAPES) if dtype == torch.float64 else len(SHAPES) // 2), exact


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_maxvol_tall(dtype):
    g = torch.Generator().manual_seed(3)
    A = torch.randn(70000, 12, generator=g, dtype=torch.float64).to(dtype)
    index, C, status = run_maxvol(A)
    check_properties(A, index[0], C[0], 1.05, dtype, "tall")
    res = host_ref(A)
    assert gaps_hold(res, torch.float64), res.min_gap()  # 5.9e-6: exact in fp64; fp32 has a decision within 1e-3
    if gaps_hold(res, dtype):
        np.testing.assert_array_equal(index[0].numpy(), res.index)
        assert int(status[0, 1]) == res.swaps


def test_maxvol_rank_limit():
    with pytest.raises(NotImplementedError, match="above 128"):
        _hip.maxvol(torch.randn(1, 300, 129, device=DEV), 1.05, 100)
    with pytest.raises(ValueError):
        _hip.maxvol(torch.randn(1, 8, 8, device=DEV), 1.05, 100)  # N > r is required of the kernel


# ------------------------------------------------------------------------------------------------------------ maxvol: batch
def _batch_items():
    """Item 0 is maximal already (0 swaps), item 1 needs many swaps, item 2 needs more than max_iters."""
    g = torch.Generator().manual_seed(21)
    N, r = 600, 16
    a0 = torch.cat([torch.eye(r, dtype=torch.float64) * 4, torch.rand(N - r, r, generator=g, dtype=torch.float64) * 2 - 1])
    a0 = a0[torch.randperm(N, generator=g)]
    heavy = lambda: torch.randn(N, r, generator=g, dtype=torch.float64) * torch.exp(torch.randn(N, 1, generator=g, dtype=torch.float64))
    items = [a0] + [heavy() for _ in range(8)]
    swaps = [ref_maxvol(a.numpy(), max_iters=1000).swaps for a in items]
    assert swaps[0] == 0
    order = sorted(range(1, 9), key=lambda k: swaps[k])
    lo, hi = next(k for k in order if swaps[k] >= 3), order[-1]
    assert swaps[hi] > swaps[lo] + 1 and swaps[lo] >= 3, swaps
    return torch.stack([a0, items[lo], items[hi]]), swaps[lo] + 1


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_maxvol_mixed_batch(dtype):
    A, it = _batch_items()
    A = A.to(dtype)
    index, C, status = run_maxvol(A, max_iters=it)
    want = [host_ref(a, max_iters=it) for a in A]
    for b in range(3):
        assert gaps_hold(want[b], dtype), (b, want[b].min_gap())
        np.testing.assert_array_equal(index[b].numpy(), want[b].index, err_msg=str(b))
        i1, C1, s1 = run_maxvol(A[b], max_iters=it)
        assert torch.equal(index[b], i1[0]) and torch.equal(C[b], C1[0]) and torch.equal(status[b], s1[0]), b
    assert status[:, 0].tolist() == [1, 1, 1]
    assert status[:, 1].tolist() == [0, want[1].swaps, it] and want[1].swaps < it


# ------------------------------------------------------------------------------------------------------------ maxvol: knobs
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_maxvol_tol_and_max_iters(dtype):
    g = torch.Generator().manual_seed(31)
    A = torch.randn(500, 20, generator=g, dtype=torch.float64).to(dtype)
    i_half, C_half, s_half = run_maxvol(A, tol=0.5)
    i_one, C_one, s_one = run_maxvol(A, tol=1.0)
    assert torch.equal(i_half, i_one) and torch.equal(C_half, C_one) and torch.equal(s_half, s_one)  # tol < 1 counts as 1
    check_properties(A, i_one[0], C_one[0], 1.0, dtype, "tol 1")
    assert int(s_one[0, 0]) == 1
    i0, C0, s0 = run_maxvol(A, max_iters=0)
    assert s0[0].tolist() == [1, 0]
    res = host_ref(A, max_iters=0)
    assert gaps_hold(res, dtype)
    np.testing.assert_array_equal(i0[0].numpy(), res.index)  # the LU start alone
    np.testing.assert_allclose(C0[0][i0[0]].double().numpy(), np.eye(20), atol=1e-4 if dtype == torch.float32 else 1e-12)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_maxvol_strided_abi(dtype):
    """stride_ab and stride_cb above N * r through the C ABI: the same rows and bitwise the same C, padding never written."""
    B, N, r, pa, pc = 3, 300, 10, 37, 53
    g = torch.Generator().manual_seed(41)
    A = torch.randn(B, N, r, generator=g, dtype=torch.float64).to(dtype)
    Ab = torch.full((B, N * r + pa), 123.0, dtype=dtype)
    Ab[:, : N * r] = A.reshape(B, -1)
    Ab = Ab.to(DEV)
    Cb = torch.full((B, N * r + pc), -5.5, dtype=dtype, device=DEV)
    index = torch.full((B, r), -1, dtype=torch.int64, device=DEV)
    status = torch.zeros(B, 2, dtype=torch.int32, device=DEV)
    L = _hip.lib()
    dt = _hip.dtype_code(dtype)
    wsb = L.ttr_maxvol_workspace_bytes(dt, N, r, B)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    rc = L.ttr_maxvol(dt, B, N, r, ctypes.c_void_p(Ab.data_ptr()), N * r + pa, ctypes.c_double(1.05), 100,
                      ctypes.c_void_p(index.data_ptr()), ctypes.c_void_p(Cb.data_ptr()), N * r + pc,
                      ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(ws.data_ptr()), wsb,
                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    Cb = Cb.cpu()
    assert bool((Cb[:, N * r:] == -5.5).all())
    i1, C1, s1 = run_maxvol(A)
    assert torch.equal(index.cpu(), i1) and torch.equal(status.cpu(), s1)
    assert torch.equal(Cb[:, : N * r].reshape(B, N, r), C1)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_maxvol_zero_column(dtype):
    """A singular input: the LU meets a zero pivot (NaN counts as 0 in every argmax, the inverse clamps its rows), so the rows
    are still distinct and in range, and the item stops."""
    g = torch.Generator().manual_seed(51)
    A = torch.randn(100, 6, generator=g, dtype=torch.float64).to(dtype)
    A[:, 2] = 0
    index, C, status = run_maxvol(A)
    assert len(set(index[0].tolist())) == 6 and 0 <= int(index.min()) and int(index.max()) < 100
    assert int(status[0, 0]) == 1


# ------------------------------------------------------------------------------------------------------------ gather step
def gather_ref(X, xrow, G, idx):
    """fp64 Y[p] = X[xrow[p]] @ G[:, idx[p], :] and |X[xrow[p]]| @ |G[:, idx[p], :]| (the error scale), in chunks of points."""
    X, G = X.double().cpu(), G.double().cpu()
    xrow = torch.arange(idx.shape[0]) if xrow is None else xrow.cpu().long()
    idx = idx.cpu().long() % G.shape[1]
    Y, S = [], []
    step = max(1, 2 ** 22 // (G.shape[0] * G.shape[2]))
    for p0 in range(0, idx.shape[0], step):
        x, s = X[xrow[p0:p0 + step]], G[:, idx[p0:p0 + step], :]
        Y.append(torch.einsum("pk,kpj->pj", x, s))
        S.append(torch.einsum("pk,kpj->pj", x.abs(), s.abs()))
    return torch.cat(Y), torch.cat(S)


def check_gather(Y, X, xrow, G, idx, what):
    ref, scale = gather_ref(X, xrow, G, idx)
    err = (Y.double().cpu() - ref).abs()
    bound = 2 * (X.shape[1] + 2) * EPS[X.dtype] * scale + 1e-300
    assert bool((err <= bound).all()), (what, float((err / bound).max()))


RANKS = (1, 31, 32, 33, 63, 64, 65, 128, 512)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_gather_step_ranks(dtype):
    """Every (r, rn) of RANKS: the 64 x 64 tiles and the k chunks of 32, with a row map that repeats rows."""
    g = torch.Generator().manual_seed(61)
    for r in RANKS:
        for rn in RANKS:
            X = torch.randn(20, r, generator=g, dtype=torch.float64).to(dtype)
            G = torch.randn(r, 3, rn, generator=g, dtype=torch.float64).to(dtype)
            xrow = torch.randint(0, 20, (65,), generator=g)
            idx = torch.randint(0, 3, (65,), generator=g)
            Y = _hip.gather_step(X.to(DEV), xrow.to(DEV), G.to(DEV), idx.to(DEV))
            check_gather(Y, X, xrow, G, idx, (r, rn))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_gather_step_points(dtype):
    g = torch.Generator().manual_seed(71)
    for P in (0, 1, 64, 65, 2 ** 17):
        for I in (1, 3, 2000):
            r, rn = (33, 65) if P < 2 ** 17 else (32, 33)
            X = torch.randn(max(P, 1), r, generator=g, dtype=torch.float64).to(dtype)
            G = torch.randn(r, I, rn, generator=g, dtype=torch.float64).to(dtype)
            xrow = torch.randint(0, max(P, 1), (P,), generator=g)
            idx = torch.randint(-I, I, (P,), generator=g)  # negative values wrap
            flag = torch.full((1,), 5, dtype=torch.int32, device=DEV)
            Y = _hip.gather_step(X.to(DEV), xrow.to(DEV), G.to(DEV), idx.to(DEV), flag=flag)
            assert tuple(Y.shape) == (P, rn) and int(flag) == 0, (P, I)
            if P:
                check_gather(Y, X, xrow, G, idx, (P, I))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_gather_step_forms(dtype):
    """int32 index vectors, G as permute(2, 1, 0) and as a slice of a larger core, X with ldx > r, out with ldy > rn (its
    padding untouched), and each output row bitwise independent of the other points."""
    g = torch.Generator().manual_seed(81)
    r, rn, I, P = 40, 70, 9, 300
    Xbig = torch.randn(50, r + 7, generator=g, dtype=torch.float64).to(dtype)
    X = Xbig[:, :r]
    Gbig = torch.randn(r + 3, I + 2, rn + 5, generator=g, dtype=torch.float64).to(dtype)
    Gs = Gbig[2:2 + r, 1:1 + I, 3:3 + rn]
    xrow = torch.randint(0, 50, (P,), generator=g, dtype=torch.int32)
    idx = torch.randint(0, I, (P,), generator=g, dtype=torch.int32)
    Xd = Xbig.to(DEV)[:, :r]
    assert Xd.stride(0) == r + 7
    out_big = torch.full((P, rn + 11), 9.0, dtype=dtype, device=DEV)
    out = out_big[:, :rn]
    Y = _hip.gather_step(Xd, xrow.to(DEV), Gbig.to(DEV)[2:2 + r, 1:1 + I, 3:3 + rn], idx.to(DEV), out=out)
    assert Y.data_ptr() == out.data_ptr()
    check_gather(Y, X, xrow, Gs, idx, "slice")
    assert bool((out_big[:, rn:] == 9).all())
    # transposed core: G [rn, I, r] viewed as [r, I, rn]
    Gt = torch.randn(rn, I, r, generator=g, dtype=torch.float64).to(dtype)
    Yt = _hip.gather_step(Xd, xrow.to(DEV), Gt.to(DEV).permute(2, 1, 0), idx.to(DEV))
    check_gather(Yt, X, xrow, Gt.permute(2, 1, 0), idx, "permute")
    # subset independence
    sub = torch.tensor([5, 0, 299, 17, 17, 123])
    Ys = _hip.gather_step(Xd, xrow[sub].to(DEV), Gt.to(DEV).permute(2, 1, 0), idx[sub].to(DEV))
    assert torch.equal(Ys.cpu(), Yt.cpu()[sub])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_gather_step_out_of_range(dtype):
    """idx >= I, idx < -I, xrow >= rows and xrow < 0 set the flag and leave `out` untouched; ranks above 512 raise."""
    g = torch.Generator().manual_seed(91)
    rows, r, I, rn, P = 30, 8, 6, 5, 70
    X = torch.randn(rows, r, generator=g, dtype=torch.float64).to(dtype).to(DEV)
    G = torch.randn(r, I, rn, generator=g, dtype=torch.float64).to(dtype).to(DEV)
    xrow = torch.randint(0, rows, (P,), generator=g)
    idx = torch.randint(0, I, (P,), generator=g)
    for what, bad_x, bad_i in (("idx = I", None, I), ("idx < -I", None, -I - 1), ("xrow = rows", rows, None),
                               ("xrow = -1", -1, None), ("xrow = -rows", -rows, None)):
        xr, ix = xrow.clone(), idx.clone()
        if bad_x is not None:
            xr[41] = bad_x
        if bad_i is not None:
            ix[66] = bad_i
        out = torch.full((P, rn), 7.0, dtype=dtype, device=DEV)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        _hip.gather_step(X, xr.to(DEV), G, ix.to(DEV), out=out, flag=flag)
        assert int(flag) == 1 and bool((out == 7).all()), what
    with pytest.raises(NotImplementedError):
        _hip.gather_step(torch.randn(4, 513, device=DEV, dtype=dtype), None, torch.randn(513, 2, 3, device=DEV, dtype=dtype),
                         torch.zeros(4, dtype=torch.int64, device=DEV))


# ------------------------------------------------------------------------------------------------------------ device cross
SQ = [2 ** 0.5, 3 ** 0.5, 5 ** 0.5, 7 ** 0.5, 11 ** 0.5, 13 ** 0.5]


def smooth(*xs):
    s = sum(SQ[k] * x for k, x in enumerate(xs))
    return torch.exp(-0.3 * sum(x * x for x in xs)) * torch.cos(3 * s) + 1 / (2 + s)


CROSS_RUNS = {
    # name: (mode sizes, ranks_tt, dtype, extra keywords).  maxvol N = r + 1 (a) and N = r (b) at bond 2; _qr_blocked above 64
    "a_n_r_plus_1": ([5, 13, 13, 5], 64, torch.float64, {}),
    "b_n_eq_r": ([5, 13, 13, 5], 65, torch.float64, {}),
    "c_r63_f32": ([64, 64, 64], 63, torch.float32, {}),
    "d_2modes_r96": ([200, 200], 96, torch.float64, {}),
    "e_5modes_r96_f32_matrix": ([16] * 5, 96, torch.float32, {"function_arg": "matrix"}),
    "f_6modes_r128": ([12] * 6, 128, torch.float64, {}),
    "g_r128_f32": ([32] * 4, 128, torch.float32, {}),
    "h_kickrank": ([10] * 4, None, torch.float64, {"kickrank": 20, "rmax": 70}),
    "i_kickrank_f32": ([24] * 3, None, torch.float32, {"kickrank": 30, "rmax": 128}),
}


def _run_cross(device, sizes, ranks, dtype, kw, seed=3):
    domain = [torch.linspace(0, 1, I, dtype=dtype, device=device) for I in sizes]
    fn = smooth
    if kw.get("function_arg") == "matrix":
        fn = lambda X: smooth(*X.t())  # noqa: E731
    torch.manual_seed(seed)
    np.random.seed(seed)
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)  # the initial cores are drawn in the default dtype
    try:
        return tn.cross(fn, domain=domain, ranks_tt=ranks, max_iter=3 if ranks is None else 2, eps=1e-30, verbose=False,
                        return_info=True, suppress_warnings=True, **kw)
    finally:
        torch.set_default_dtype(old)


def check_fibres(t, info, values_at, dtype, name):
    """t[i0, rsets[0][a]] = f at those grid points, for every i0 and every row a of the final right set of bond 0."""
    rs = np.asarray(info["rsets"][0])
    I0, N = t.shape[0], t.dim()
    assert rs.shape[1] == N and not rs[:, -1].any(), name  # modes 1 .. N-1, then the reference's zero column
    assert all(0 <= rs[:, k].min() and rs[:, k].max() < t.shape[k + 1] for k in range(N - 1)), name
    assert len(np.unique(rs, axis=0)) == len(rs), name
    pts = [np.repeat(np.arange(I0), len(rs))] + [np.tile(rs[:, k], I0) for k in range(N - 1)]
    got = t[[torch.as_tensor(p, device=DEV) for p in pts]].torch().double().cpu()
    want = values_at(pts)
    tol = 1e-9 if dtype == torch.float64 else 1e-4
    err = float((got - want).abs().max() / want.abs().max())
    assert err <= tol, (name, err)


def check_sets(info, sizes, name):
    for n, s in enumerate(info["lsets"][1:], start=1):
        s = np.asarray(s)
        assert len(np.unique(s, axis=0)) == len(s), (name, "lset", n)
        assert all(0 <= s[:, k].min() and s[:, k].max() < sizes[k - 1] for k in range(1, s.shape[1])), (name, n)
    for n, s in enumerate(info["rsets"][:-1]):
        s = np.asarray(s)
        assert len(np.unique(s, axis=0)) == len(s) and not s[:, -1].any(), (name, "rset", n)
        assert all(0 <= s[:, k].min() and s[:, k].max() < sizes[n + 1 + k] for k in range(s.shape[1] - 1)), (name, n)


@pytest.mark.parametrize("name", sorted(CROSS_RUNS))
def test_cross_device_interpolates(name):
    sizes, ranks, dtype, kw = CROSS_RUNS[name]
    t, info = _run_cross(DEV, sizes, ranks, dtype, kw)
    assert t.cores[0].device.type == "cuda" and t.cores[0].dtype == dtype
    grids = [np.linspace(0, 1, I) for I in sizes]
    check_fibres(t, info, lambda pts: smooth(*[torch.as_tensor(g[p]) for g, p in zip(grids, pts)]), dtype, name)
    check_sets(info, sizes, name)
    # the validation error of a host cross with the same draws; the floor is the dtype's rounding of the samples
    th, ih = _run_cross("cpu", sizes, ranks, torch.float64, kw)
    v_dev, v_host = float(info["val_epss"][-1]), float(ih["val_epss"][-1])
    assert v_dev <= 10 * v_host + 100 * EPS[dtype], (name, v_dev, v_host)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_cross_device_tensors(dtype):
    """tensors=[t1, t2]: f of two random trains, checked at the fibres against the trains' own values."""
    g = torch.Generator().manual_seed(17)
    mk = lambda r: tn.Tensor([torch.randn(a, 11, b, generator=g, dtype=torch.float64)  # noqa: E731
                              for a, b in zip([1, r, r, r], [r, r, r, 1])])
    t1, t2 = mk(5), mk(7)
    f = lambda x, y: x * y + x  # noqa: E731
    torch.manual_seed(5)
    np.random.seed(5)
    t, info = tn.cross(f, tensors=[tn.Tensor([c.to(DEV, dtype) for c in s.cores]) for s in (t1, t2)], ranks_tt=40, max_iter=2,
                       eps=1e-30, verbose=False, return_info=True, suppress_warnings=True)
    d1, d2 = t1.torch(), t2.torch()
    check_fibres(t, info, lambda pts: f(d1[tuple(pts)], d2[tuple(pts)]), dtype, "tensors")
    check_sets(info, [11] * 4, "tensors")


def test_cross_device_rank_limit():
    """Ranks above 128 on device cores: NotImplementedError before the function is called (fixed ranks), or at the augmentation
    that would pass the limit (adaptive), instead of a maxvol failure in the middle of a sweep."""
    calls = []

    def f(*xs):
        calls.append(1)
        return smooth(*xs)

    domain = [torch.linspace(0, 1, 64, device=DEV) for _ in range(4)]
    with pytest.raises(NotImplementedError, match="128"):
        tn.cross(f, domain=domain, ranks_tt=130, verbose=False)
    assert len(calls) == 0
    tn.cross(f, domain=domain, ranks_tt=128, max_iter=1, verbose=False, suppress_warnings=True)  # the limit itself runs
    calls.clear()
    with pytest.raises(NotImplementedError, match="128"):
        tn.cross(f, domain=domain, kickrank=130, rmax=200, max_iter=3, eps=1e-30, verbose=False)
    assert len(calls) == 1 + 7  # the validation set and one sweep of 4 modes at rank 1

"""ttr_sparse_gram / ttr_sparse_project against fp64 dense products of an explicitly built D, and tn.sparse_tt_svd end to end on
the device.

Bounds.  Every element of G and W is one ordered fma chain (plus, for a split i list, the sum of its parts in order), so its
error is at most L eps sum |terms| with L the number of terms (Higham, Accuracy and Stability, (3.5)); for the Gram matrix
sum |terms| <= sqrt(G_ii G_jj) <= max |G|, for the projection it is (|D|^T |U|) elementwise.  L is taken as the longest sum.
"""
import os

import numpy as np
import pytest
import torch

import tntorch_amd as tn
from tntorch_amd import _hip, interpolation

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
RANKS, SIZES = (1, 3, 16, 17, 33), (1, 5, 16, 67)
FILLINGS = ("one_block", "one_full_column", "absent_index", "one_column")
EPS = {torch.float32: 2.0**-24, torch.float64: 2.0**-53}  # unit roundoff


def golden_case(name):
    from test_sparse_host import golden_case as g

    return g(name)


def golden_bound(name):
    from test_sparse_host import golden_bound as g

    return g(name)


def table(r, I, filling, dtype, seed, C=23):
    """A block table on the CPU and its dense D (fp64): (colptr, blk_i, blkcol, V, D, longest column)."""
    g = torch.Generator().manual_seed(seed)
    cols = []
    C = 1 if filling == "one_column" else C
    for c in range(C):
        if filling == "one_block":
            idx = torch.randint(0, I, (1,), generator=g)
        elif filling == "one_full_column" and c == C // 2:
            idx = torch.arange(I)
        else:
            m = int(torch.randint(1, min(I, 6) + 1, (1,), generator=g))
            idx = torch.randperm(I, generator=g)[:m].sort().values
        if filling == "absent_index" and I > 1:
            idx = idx[idx != I // 2]
            if idx.numel() == 0:
                idx = torch.tensor([0])
        cols.append(idx)
    blk_i = torch.cat(cols)
    counts = torch.tensor([len(c) for c in cols])
    colptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(counts, 0)])
    blkcol = torch.repeat_interleave(torch.arange(C), counts)
    V = torch.randn(blk_i.numel(), r, generator=g, dtype=torch.float64).to(dtype)
    D = torch.zeros(r * I, C, dtype=torch.float64)
    D[torch.arange(r)[None, :] * I + blk_i[:, None], blkcol[:, None].expand(-1, r)] = V.double()
    return colptr, blk_i, blkcol, V, D, int(counts.max())


def device_gram(colptr, blk_i, blkcol, V, I):
    order = torch.sort(blk_i, stable=True).indices
    iptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.bincount(blk_i, minlength=I), 0)])
    ilist, ip = _hip.sparse_group(blk_i.to(DEV, torch.int32), I)  # the device's stable counting sort against torch's
    assert torch.equal(ilist.cpu().long(), order) and torch.equal(ip.cpu().long(), iptr)
    return _hip.sparse_gram(V.to(DEV), I, colptr.to(DEV), blk_i.to(DEV), blkcol.to(DEV), ilist, ip)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("filling", FILLINGS)
def test_gram_and_project_against_dense(filling, dtype):
    for r in RANKS:
        for I in SIZES:
            colptr, blk_i, blkcol, V, D, mmax = table(r, I, filling, dtype, 100 * r + I)
            n, C = r * I, colptr.numel() - 1
            if n > _hip.max_eigh_n(dtype):  # outside the envelope (fp64: 2048 rows)
                with pytest.raises(NotImplementedError):
                    device_gram(colptr, blk_i, blkcol, V, I)
                continue
            G = device_gram(colptr, blk_i, blkcol, V, I)
            ref = D @ D.t()
            L = C  # an element sums at most one term per column
            err, bound = float((G.cpu().double() - ref).abs().max()), L * EPS[dtype] * float(ref.abs().max())
            assert err <= bound, (r, I, err, bound)
            assert torch.equal(G, G.t()), (r, I)
            assert torch.equal(G, device_gram(colptr, blk_i, blkcol, V, I)), (r, I)  # run to run
            absent = torch.bincount(blk_i, minlength=I) == 0
            if bool(absent.any()):
                rows = (torch.arange(r)[:, None] * I + torch.nonzero(absent)[:, 0][None, :]).reshape(-1).to(DEV)
                assert float(G[rows].abs().max()) == 0.0 and float(G[:, rows].abs().max()) == 0.0, (r, I)
            # the projection onto q columns of an orthonormal U, read through strides (a transposed view)
            q = min(n, 7)
            U = torch.linalg.qr(torch.randn(n, n, generator=torch.Generator().manual_seed(r + I), dtype=torch.float64)).Q.to(dtype)
            Ud = U.t().contiguous().to(DEV).t()
            W = _hip.sparse_project(V.to(DEV), I, colptr.to(DEV), blk_i.to(DEV), Ud, q)
            refw = D.t() @ U.double()[:, :q]
            scale = D.abs().t() @ U.double().abs()[:, :q]
            Lw = mmax * r
            assert bool(((W.cpu().double() - refw).abs() <= Lw * EPS[dtype] * scale + 1e-300).all()), (r, I)
            assert torch.equal(W, _hip.sparse_project(V.to(DEV), I, colptr.to(DEV), blk_i.to(DEV), Ud, q)), (r, I)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("r,I,nb", [(3, 1, 5000), (2, 2, 9000)])
def test_gram_of_an_i_list_split_into_partials(r, I, nb, dtype):
    """Every column holds one block, so mode index i's list has ~nb / I entries: several parts, summed in part order."""
    assert _hip.sparse_gram_parts(dtype, r, I, nb) == 3
    g = torch.Generator().manual_seed(nb)
    blk_i = torch.randint(0, I, (nb,), generator=g)
    colptr, blkcol = torch.arange(nb + 1), torch.arange(nb)
    V = torch.randn(nb, r, generator=g, dtype=torch.float64).to(dtype)
    D = torch.zeros(r * I, nb, dtype=torch.float64)
    D[torch.arange(r)[None, :] * I + blk_i[:, None], blkcol[:, None].expand(-1, r)] = V.double()
    G = device_gram(colptr, blk_i, blkcol, V, I)
    ref = D @ D.t()
    L = int(torch.bincount(blk_i, minlength=I).max())
    assert float((G.cpu().double() - ref).abs().max()) <= L * EPS[dtype] * float(ref.abs().max())
    assert torch.equal(G, G.t()) and torch.equal(G, device_gram(colptr, blk_i, blkcol, V, I))


def test_shuffled_samples_give_bit_identical_cores():
    X, y = golden_case("s200")[:2]
    for dtype in (torch.float32, torch.float64):
        a = tn.sparse_tt_svd(X.to(DEV), y.to(DEV, dtype), 0.05)
        p = torch.randperm(X.shape[0], generator=torch.Generator().manual_seed(1))
        b = tn.sparse_tt_svd(X[p].to(DEV), y[p].to(DEV, dtype), 0.05)
        assert len(a.cores) == len(b.cores) and all(torch.equal(u, v) for u, v in zip(a.cores, b.cores))


@pytest.mark.parametrize("name", ["dense", "s200", "s200r", "n2"])
def test_golden_on_the_device(name):
    X, y, eps, rmax, ranks, recon = golden_case(name)
    t = tn.sparse_tt_svd(X.to(DEV), y.to(DEV), eps, rmax=rmax)
    assert all(c.is_cuda and c.dtype == torch.float64 for c in t.cores)
    mirror = tn.sparse_tt_svd(X, y, eps, rmax=rmax)
    assert [int(r) for r in t.ranks_tt] == ranks == [int(r) for r in mirror.ranks_tt]
    dist = float(torch.norm(t.torch().cpu() - recon) / torch.norm(y))
    print(name, "device distance from the reference's reconstruction / ||y|| =", dist, "bound", golden_bound(name))
    assert dist <= golden_bound(name)


@pytest.mark.parametrize("eps", [0.3, 0.05])
@pytest.mark.parametrize("name", ["dense", "s200"])
def test_eps_guarantee_fp32(name, eps):
    X, y = golden_case(name)[:2]
    y = y.float()
    t = tn.sparse_tt_svd(X.to(DEV), y.to(DEV), eps)
    assert all(c.dtype == torch.float32 for c in t.cores)
    D = torch.zeros(6, 5, 7, 4, dtype=torch.float64)
    D[tuple(X.t())] = y.double()
    err = float(torch.norm(t.torch().cpu().double() - D) / torch.norm(D))
    print(name, eps, "ranks", t.ranks_tt.tolist(), "relative error", err)
    assert err <= eps * (1 + 1e-6)


def test_small_and_mixed_inputs():
    # P = 1, N = 2
    t = tn.sparse_tt_svd(torch.tensor([[2, 1]], device=DEV), torch.tensor([3.0], dtype=torch.float64, device=DEV), 0.1, shape=[4, 3])
    full = t.torch().cpu()
    assert [int(r) for r in t.ranks_tt] == [1, 1, 1] and float(full[2, 1]) == pytest.approx(3.0, rel=1e-14)
    full[2, 1] = 0
    assert float(full.abs().max()) == 0.0
    # int32 X; NumPy X with the device chosen by y; NumPy both -> CPU
    X, y, eps, rmax, ranks, recon = golden_case("s200")
    a = tn.sparse_tt_svd(X.to(DEV, torch.int32), y.to(DEV), eps)
    b = tn.sparse_tt_svd(X.numpy(), y.to(DEV), eps)
    c = tn.sparse_tt_svd(X.numpy(), y.numpy(), eps)
    assert all(k.is_cuda for k in a.cores + b.cores) and not any(k.is_cuda for k in c.cores)
    assert [int(r) for r in a.ranks_tt] == ranks == [int(r) for r in b.ranks_tt]
    assert all(torch.equal(u, v) for u, v in zip(a.cores, b.cores))


def test_dense_unfolding_is_never_built(monkeypatch):
    """[128, 64, 64, 64], 2^18 distinct positions, rmax = 4: the peak of device memory up to the end of step 1, X and y included,
    stays under a quarter of that step's dense D (128 x ncols), with torch's dense products and torch.linalg patched out.  The
    peaks of every step are printed."""
    g = torch.Generator().manual_seed(5)
    shape, P = [128, 64, 64, 64], 1 << 18
    flat = torch.randperm(int(np.prod(shape)), generator=g)[:P]
    X = torch.stack(torch.unravel_index(flat, shape), dim=1).to(DEV)
    y = torch.randn(P, generator=g).to(DEV)
    ncols = len(torch.unique(flat % (64**3)))  # flat = x_1 64^3 + (suffix)
    dense_bytes = 128 * ncols * 4

    def banned(*a, **k):
        raise AssertionError("a dense torch product reached by a device sparse_tt_svd")

    for name in ("einsum", "matmul", "bmm", "mm"):
        monkeypatch.setattr(torch, name, banned)
    monkeypatch.setattr(torch.Tensor, "__matmul__", banned)
    for name in [n for n in dir(torch.linalg) if not n.startswith("_") and callable(getattr(torch.linalg, n))]:
        monkeypatch.setattr(torch.linalg, name, banned)
    peaks = []

    def hook(n):
        peaks.append(torch.cuda.max_memory_allocated())
        torch.cuda.reset_peak_memory_stats()

    monkeypatch.setattr(interpolation, "_STEP_HOOK", hook)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t = tn.sparse_tt_svd(X, y, 1e-3, shape=shape, rmax=4)
    torch.cuda.synchronize()
    monkeypatch.undo()
    print("dense D of step 1: {} bytes ({} columns); inputs {} bytes; peak per step {}".format(dense_bytes, ncols, base, peaks))
    assert len(peaks) == 3 and max(int(r) for r in t.ranks_tt) <= 4
    # X and y count; only what other tests left allocated at entry does not
    assert peaks[0] - (base - X.nbytes - y.nbytes) < dense_bytes / 4, (peaks, base, dense_bytes)


def test_envelope_raises_before_any_kernel(monkeypatch):
    def banned(*a, **k):
        raise AssertionError("a kernel was launched")

    monkeypatch.setattr(_hip, "_call", banned)
    X = torch.tensor([[0, 0, 0], [1, 4099, 1]], device=DEV)
    y = torch.ones(2, device=DEV)
    with pytest.raises(NotImplementedError, match="bond 2"):
        tn.sparse_tt_svd(X, y, 0.1, shape=[4, 4100, 2], rmax=2)  # 2 x 4100 rows at bond 2
    with pytest.raises(NotImplementedError, match="bond 1"):
        tn.sparse_tt_svd(X, y.double(), 0.1, shape=[2049, 4100, 2], rmax=2)


def test_bad_indices_set_the_flag_and_write_nothing():
    X = torch.tensor([[0, 1, 2], [1, 0, 1], [2, 2, 0]], device=DEV)
    y = torch.tensor([1.0, 2.0, 3.0], device=DEV)
    shape = torch.tensor([3, 3, 3], device=DEV)
    for bad_value in (-1, 3):
        bad = X.clone()
        bad[1, 2] = bad_value
        with pytest.raises(ValueError):
            tn.sparse_tt_svd(bad, y, 0.1, shape=[3, 3, 3])
        flag = torch.full((1,), 7, dtype=torch.int32, device=DEV)
        key = torch.full((3,), -5, dtype=torch.int64, device=DEV)
        _hip._call("ttr_sparse_keys", 3, 3, bad.data_ptr(), 3, 1, shape.data_ptr(), key.data_ptr(), flag.data_ptr())
        lev = torch.full((3,), -5, dtype=torch.int32, device=DEV)
        _hip._call("ttr_sparse_levels", 3, 3, bad.data_ptr(), 3, 1, torch.arange(3, device=DEV, dtype=torch.int32).data_ptr(), lev.data_ptr(),
                   flag.data_ptr())
        assert int(flag) == 1 and key.tolist() == [-5] * 3 and lev.tolist() == [-5] * 3
    with pytest.raises(ValueError):
        tn.sparse_tt_svd(torch.cat([X, X[:1]]), torch.cat([y, y[:1]]), 0.1)  # a repeated position
    flag = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    key = _hip.sparse_keys(X, shape, flag)
    assert int(flag) == 0 and key.tolist() == [0 + 3 * 1 + 9 * 2, 1 + 0 + 9 * 1, 2 + 3 * 2 + 0]
    lev = _hip.sparse_levels(X, torch.sort(key).indices.to(torch.int32), flag)
    assert int(flag) == 0 and lev.tolist() == [3, 3, 3]

"""Indexing on device cores: the golden replay of test_indexing_host.py, ttr_gather_chain through the C ABI against an fp64
CPU chain, bitwise subset independence, device-side index validation, the metric shape, and the no-torch-linear-algebra rule."""
import pytest
import torch

import tntorch_amd as tn
from tntorch_amd import _hip, _hostops
from test_indexing_host import replay

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def cores_for(ranks, I, B, dtype, seed, dev=DEV):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(B, ranks[n], I, ranks[n + 1], generator=g, dtype=torch.float64) / ranks[n] ** 0.5).to(dev, dtype)
            for n in range(len(ranks) - 1)]


def cpu_chain(cores, cols):
    return _hostops.gather_chain([c.double().cpu() for c in cores], [i.long().cpu() for i in cols])


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def test_golden_replay_device():
    assert replay(DEV) == 88


CASES = [(R, N, P) for R in (1, 3, 16, 64, 65, 128, 512) for N in (2, 8) for P in (1, 17, 256)]
CASES += [(R, N, 100000) for R in (1, 3, 16) for N in (2, 8)] + [(64, 2, 100000)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("R,N,P", CASES)
def test_gather_chain_whole_train(R, N, P, dtype):
    I = 5
    ranks = [1] + [R] * (N - 1) + [1]
    cores = cores_for(ranks, I, 1, dtype, seed=R * 100 + N)
    g = torch.Generator().manual_seed(P)
    cols = [torch.randint(-I, I, (P,), generator=g).to(DEV) for _ in range(N)]  # negative entries wrap
    out = _hip.gather_chain(cores, cols)
    assert out.shape == (1, 1, P, 1)
    assert rel(out, cpu_chain(cores, cols)) <= (2e-5 if dtype == torch.float32 else 1e-12)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
def test_gather_chain_batch_mid_train_strided(dtype, idx_dtype):
    """B > 1, a block with r_a, r_b > 1, non-contiguous cores, index columns of a [P, N] matrix (stride N), repeated indices."""
    B, I, P = 3, 7, 3000
    ranks = [4, 65, 16, 33, 5]
    base = cores_for(ranks, I, B, dtype, seed=3)
    cores = [c.transpose(2, 3).contiguous().transpose(2, 3) for c in base]  # same values, I-stride 1
    g = torch.Generator().manual_seed(5)
    M = torch.randint(0, 3, (P, len(cores)), generator=g).to(DEV, idx_dtype)  # only 3 of 7 values: many repeats
    cols = [M[:, n] for n in range(len(cores))]
    for dm in (-1, 0, 1 << 40):
        out = _hip.gather_chain(cores, cols, direct_max_points=dm)
        assert out.shape == (B, 4, P, 5)
        assert rel(out, cpu_chain(base, cols)) <= (2e-5 if dtype == torch.float32 else 1e-12)


def test_gather_chain_skewed_and_paths_bitwise():
    """All points on one index value; the sorted and the direct path give bitwise the same values."""
    I, P = 9, 5000
    cores = cores_for([1, 64, 64, 64, 1], I, 2, torch.float32, seed=7)
    cols = [torch.full((P,), 4, device=DEV, dtype=torch.int64) for _ in range(4)]
    cols[1][::7] = 2
    a = _hip.gather_chain(cores, cols, direct_max_points=0)
    b = _hip.gather_chain(cores, cols, direct_max_points=1 << 40)
    assert torch.equal(a, b)
    assert rel(a, cpu_chain(cores, cols)) <= 2e-5


def test_subset_independence_bitwise():
    I, P = 16, 20000
    cores = cores_for([2, 64, 65, 128, 3], I, 1, torch.float32, seed=11)
    g = torch.Generator().manual_seed(12)
    cols = [torch.randint(0, I, (P,), generator=g).to(DEV) for _ in range(4)]
    full = _hip.gather_chain(cores, cols)
    for k in (1, 17, 256, 3000):
        sel = torch.randperm(P, generator=g)[:k].to(DEV)
        part = _hip.gather_chain(cores, [c[sel] for c in cols])
        assert torch.equal(part, full[:, :, sel, :]), k


def test_out_of_range_on_device():
    I, P = 6, 1000
    cores = cores_for([1, 8, 8, 1], I, 1, torch.float64, seed=13)
    for bad in (I, -I - 1):
        cols = [torch.randint(0, I, (P,), device=DEV) for _ in range(3)]
        cols[2][P // 2] = bad
        out = torch.full((1, 1, P, 1), 123.0, dtype=torch.float64, device=DEV)
        with pytest.raises(IndexError):
            _hip.gather_chain(cores, cols, out=out)
        assert bool((out == 123.0).all())  # nothing written after the check failed
        t = tn.Tensor([c[0] for c in cores])
        with pytest.raises(IndexError):
            t[torch.stack(cols, 1)]
    cols = [torch.randint(0, I, (P,), device=DEV) for _ in range(3)]  # and the device is fine afterwards
    assert rel(_hip.gather_chain(cores, cols), cpu_chain(cores, cols)) <= 1e-12


def test_metric_shape_against_host_mirror():
    N, I, R, P = 8, 64, 64, 1 << 16
    ranks = [1] + [R] * (N - 1) + [1]
    cores = cores_for(ranks, I, 1, torch.float32, seed=17)
    t = tn.Tensor([c[0] for c in cores])
    h = tn.Tensor([c[0].cpu().double() for c in cores])
    idx = torch.randint(0, I, (P, N), device=DEV)
    got = t[idx]
    assert [tuple(c.shape) for c in got.cores] == [(1, P, 1)] and got.cores[0].is_cuda
    ic = idx.cpu()
    want = torch.cat([h[ic[s:s + 4096]].cores[0] for s in range(0, P, 4096)], 1)
    assert rel(got.cores[0], want) <= 1e-5


def test_device_call_uses_no_torch_linear_algebra(monkeypatch):
    t = tn.Tensor([c[0] for c in cores_for([1, 5, 6, 7, 1], 6, 1, torch.float64, seed=19)])
    tk = tn.Tensor([c[0] for c in cores_for([1, 5, 6, 7, 1], 4, 1, torch.float64, seed=20)],
                   Us=[torch.randn(6, 4, dtype=torch.float64, device=DEV), None, torch.randn(8, 4, dtype=torch.float64, device=DEV), None])
    keys = [(0, [1, 2], [3, 3]), (1, 2, 3, 3), (slice(None), 2), (None, ..., 1), torch.randint(0, 4, (50, 4), device=DEV),
            ([0, 1], 2, slice(None), 1), (2, slice(None), [0, 3], [1, 1])]
    want = [[t[k], tk[k]] for k in keys]

    def boom(*a, **k):
        raise AssertionError("torch linear algebra on a device call")

    monkeypatch.setattr(torch, "einsum", boom)
    monkeypatch.setattr(torch, "matmul", boom)
    monkeypatch.setattr(torch, "bmm", boom)
    monkeypatch.setattr(torch.Tensor, "__matmul__", boom)
    for k, (a, b) in zip(keys, want):
        for x, w in ((t, a), (tk, b)):
            r = x[k]
            rv = r if isinstance(r, torch.Tensor) else r.cores[0]
            wv = w if isinstance(w, torch.Tensor) else w.cores[0]
            assert rv.is_cuda and torch.equal(rv, wv)

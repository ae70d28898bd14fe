"""The host side of a rounding call on the device: a sweep that ttr_round_tt declines after it has enqueued work, an exception in
a later sub-batch, and the three paths `truncate` dispatches to."""
import pytest
import torch

from parity import rel_diff
from tntorch_amd import _hip, _hipops

pytestmark = pytest.mark.gpu


def _train(B, N, I, r, dt, seed):
    """[B, r0, I, r1] cores with inner ranks ``r`` and boundary ranks 1 and 2.  (The right boundary rank: ttr_round_tt only takes
    trains whose every bond has rows <= columns, and with a boundary rank of 1 the last bond of these small trains is r x I > I.)"""
    g = torch.Generator().manual_seed(seed)
    rk = [1] + [r] * (N - 1) + [2]
    return [torch.randn(B, rk[mu], I, rk[mu + 1], generator=g, dtype=torch.float64).to(dt).cuda() for mu in range(N)]


def _spy_release(monkeypatch):
    """(polled?, the words as they were) at every release of a host word."""
    seen = []
    orig = _hipops._HostWords._release
    monkeypatch.setattr(_hipops._HostWords, "_release", lambda self, w: seen.append((w.event is None, w.host.clone())) or orig(self, w))
    return seen


@pytest.mark.parametrize("dt,B,batch", [(torch.float32, 3, True), (torch.float64, 1, False)])
def test_sweep_declined_after_it_ran_falls_back_with_its_word_written(dt, B, batch, monkeypatch):
    """ttr_round_tt returns TTR_E_UNSUPPORTED from inside the sweep (here: after ALL of it was enqueued): the host loop gives the
    host loop's cores, and the pinned word of the declined call is released only after the device has written it."""
    cores = _train(B, 4, 4, 8, dt, seed=1)
    eps, rmax = (None if batch else 1e-6), [4, 4, 4]
    monkeypatch.setattr(_hipops, "SWEEP_C_ENABLED", False)
    ref = _hipops.round_tt(cores, eps, rmax, "svd", batch)
    monkeypatch.setattr(_hipops, "SWEEP_C_ENABLED", True)
    real, declined = _hip.round_tt_sweep, []

    def decline(*a):
        real(*a)
        declined.append(a[9])                       # (the zero_flag argument: the pinned words)
        raise NotImplementedError("declined by the test")

    monkeypatch.setattr(_hip, "round_tt_sweep", decline)
    released = _spy_release(monkeypatch)
    n0 = _hipops.SWEEP_C_CALLS
    out = _hipops.round_tt(cores, eps, rmax, "svd", batch)
    assert len(declined) == 1 and declined[0] is not None and _hipops.SWEEP_C_CALLS == n0
    assert [tuple(x.shape) for x in out] == [tuple(x.shape) for x in ref]
    assert all(torch.equal(x, y) for x, y in zip(out, ref))
    polled = [h for is_polled, h in released if is_polled]
    assert len(polled) == 1 and polled[0].numel() == (1 if batch else 3)
    assert (polled[0] != _hipops._ZF_PENDING).all()


def test_exception_in_a_later_chunk_leaves_no_word_pending(monkeypatch):
    """B = 130 runs as two sub-batches on two streams.  The second one raises: the error reaches the caller, the first one's
    zero-guard word was written before it was released, and the next call is not disturbed."""
    cores = _train(130, 3, 3, 4, torch.float32, seed=2)
    rmax = [2, 2]
    monkeypatch.setattr(_hipops, "STREAM_CHUNKS_ENABLED", False)
    ref = _hipops.round_tt(cores, None, rmax, "svd", True)
    monkeypatch.setattr(_hipops, "STREAM_CHUNKS_ENABLED", True)
    real, calls = _hipops._round_tt_sweep, []

    def second_fails(*a):
        calls.append(a[0][0].shape[0])
        if len(calls) == 2:
            raise RuntimeError("second chunk")
        return real(*a)

    released = _spy_release(monkeypatch)
    with monkeypatch.context() as m:
        m.setattr(_hipops, "_round_tt_sweep", second_fails)
        with pytest.raises(RuntimeError, match="second chunk"):
            _hipops.round_tt(cores, None, rmax, "svd", True)
    assert calls == [65, 65]
    assert len(released) == 1 and all((h != _hipops._ZF_PENDING).all() for _, h in released)
    out = _hipops.round_tt(cores, None, rmax, "svd", True)
    assert len(released) == 3
    assert all(torch.equal(x, y) for x, y in zip(out, ref))


def _with_spectrum(B, m, n, dt, seed):
    """[B, m, n] with singular values 1, .9, .8, .7 | .25, .2, ... (x 0.8 each): a cut at 4 with a gap of a factor 2.8, so the
    rank-4 truncation is determined to a few eps of the dtype."""
    g = torch.Generator().manual_seed(seed)
    k = min(m, n)
    s = torch.cat([torch.tensor([1.0, 0.9, 0.8, 0.7]), 0.25 * 0.8 ** torch.arange(k - 4)]).double()
    out = []
    for _ in range(B):
        U = torch.linalg.qr(torch.randn(m, k, generator=g, dtype=torch.float64))[0]
        V = torch.linalg.qr(torch.randn(n, k, generator=g, dtype=torch.float64))[0]
        out.append((U * s) @ V.T)
    return torch.stack(out).to(dt)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
@pytest.mark.parametrize("left_ortho", [False, True])
@pytest.mark.parametrize("shape,path", [((8, 24), "rows64"), ((40, 8), "cols64"), ((72, 80), "gemm")])
def test_truncate_dispatches_by_shape_and_matches_lapack(shape, path, left_ortho, dt, monkeypatch):
    """Up to 64 rows -> the fused row sweep, tall with up to 64 columns -> the fused column sweep, else the GEMM path (whose range
    finder may hand a projected 32-row problem to the row sweep afterwards).  Batch mode, B = 2, rank cap 4; the product of the
    factors against LAPACK's truncation of the same matrix, at the bound of `test_big_bond_range_finder_vs_lapack`."""
    seen = []
    for name in ("rows64", "cols64", "gemm"):
        real = getattr(_hipops, "_truncate_" + name)
        monkeypatch.setattr(_hipops, "_truncate_" + name, lambda *a, _n=name, _f=real: seen.append(_n) or _f(*a))
    M = _with_spectrum(2, *shape, dt, seed=7)
    t = _hipops.truncate(M.cuda(), None, 4, left_ortho, "svd", True)
    assert seen[0] == path and (path == "gemm" or seen == [path]), seen
    assert t.rank == 4 and not t.zero
    ours = (t.left_scaled() @ t.right).cpu()
    U, S, Vh = torch.linalg.svd(M.double(), full_matrices=False)
    ref = (U[:, :, :4] * S[:, None, :4]) @ Vh[:, :4]
    for i in range(2):
        assert rel_diff(ours[i], ref[i]) <= (1e-5 if dt == torch.float32 else 1e-11)
    orth = t.left if left_ortho else t.right.transpose(1, 2)
    eye = torch.eye(4, dtype=torch.float64)
    assert ((orth.cpu().double().transpose(1, 2) @ orth.cpu().double()) - eye).abs().max().item() <= (3e-5 if dt == torch.float32 else 1e-11)

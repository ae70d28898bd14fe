"""The host side of a rounding call without a GPU: the owner of the host words that the device writes asynchronously
(`_hipops._HostWords`), the one eps-deferral policy both sweeps ask, and the zero-train builder."""
import threading
import time
import types

import pytest
import torch

from tntorch_amd import _hipops
from tntorch_amd._hipops import _ZF_PENDING, _HostWords


class FakeStream:
    def __init__(self, on_sync=None):
        self.syncs, self.on_sync = 0, on_sync

    def synchronize(self):
        self.syncs += 1
        if self.on_sync is not None:
            self.on_sync()


def _spy_release(monkeypatch):
    """Every release of a host word, with the words as they were at that moment."""
    seen = []
    orig = _HostWords._release
    monkeypatch.setattr(_HostWords, "_release", lambda self, w: seen.append(w.host.clone()) or orig(self, w))
    return seen


def test_written_word_is_returned_without_a_synchronise():
    st = FakeStream()
    host = torch.zeros(3, dtype=torch.int32)
    with _HostWords() as words:
        w = words.polled(host, st)
        assert host.tolist() == [_ZF_PENDING] * 3
        threading.Timer(0.02, lambda: host.copy_(torch.tensor([5, 0, 7], dtype=torch.int32))).start()
        assert words.wait(w).tolist() == [5, 0, 7]
        assert words.open == []
    assert st.syncs == 0


def test_unwritten_word_raises_after_one_synchronise(monkeypatch):
    monkeypatch.setattr(_hipops, "_HOST_WORD_TIMEOUT_S", 0.005)
    st = FakeStream()
    with _HostWords() as words:
        w = words.polled(torch.zeros(2, dtype=torch.int32), st)
        with pytest.raises(RuntimeError, match="TTR_ABI_VERSION") as ei:
            words.wait(w)
        assert "did not write" in str(ei.value)
        assert words.open == []          # released: the stream has been synchronised, nothing can land later
    assert st.syncs == 1


def test_a_word_the_synchronise_completes_is_a_value(monkeypatch):
    """The fallback itself is not an error: what the kernel wrote by the time its stream has drained is the answer."""
    monkeypatch.setattr(_hipops, "_HOST_WORD_TIMEOUT_S", 0.005)
    host = torch.zeros(1, dtype=torch.int32)
    st = FakeStream(on_sync=lambda: host.fill_(4))
    with _HostWords() as words:
        assert words.wait(words.polled(host, st)).tolist() == [4]
    assert st.syncs == 1


@pytest.mark.parametrize("leave", ["exception", "normal"])
def test_leaving_with_unwaited_words_drains_them_first(leave, monkeypatch):
    """Two words issued, none waited for: one is written shortly after, the other only by the time its stream has drained.  Both
    carry their values when they are released, and that happens before the block is left -- with the caller's exception intact."""
    monkeypatch.setattr(_hipops, "_HOST_WORD_TIMEOUT_S", 0.05)
    released = _spy_release(monkeypatch)
    a, b = torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    sa, sb = FakeStream(), FakeStream(on_sync=lambda: b.fill_(9))
    left = []

    def body():
        with _HostWords() as words:
            words.polled(a, sa)
            words.polled(b, sb)
            threading.Timer(0.01, lambda: a.fill_(3)).start()
            if leave == "exception":
                raise KeyError("from the caller")
        left.append(len(released))

    if leave == "exception":
        with pytest.raises(KeyError, match="from the caller"):
            body()
    else:
        body()
        assert left == [2]
    assert [r.tolist() for r in released] == [[3], [9, 9]]     # nothing pending at its release
    assert (sa.syncs, sb.syncs) == (0, 1)


def test_interrupted_drain_synchronises_the_stream(monkeypatch):
    """A KeyboardInterrupt inside the poll of the drain: the word's stream is synchronised instead, the word is released written,
    and the interrupt is not swallowed."""
    host = torch.zeros(1, dtype=torch.int32)
    st = FakeStream(on_sync=lambda: host.fill_(1))
    released = _spy_release(monkeypatch)

    def interrupted(self, w):
        raise KeyboardInterrupt

    monkeypatch.setattr(_HostWords, "_settle", interrupted)
    with pytest.raises(KeyboardInterrupt):
        with _HostWords() as words:
            words.polled(host, st)
    assert st.syncs == 1 and [r.tolist() for r in released] == [[1]]


def test_abandoned_word_is_synchronised_not_read():
    host = torch.zeros(1, dtype=torch.int32)
    st = FakeStream()
    with _HostWords() as words:
        words.abandon(words.polled(host, st))
        assert words.open == [] and st.syncs == 1
    assert st.syncs == 1


def test_polling_yields_after_the_tight_phase(monkeypatch):
    monkeypatch.setattr(_hipops, "_HOST_WORD_TIGHT_POLLS", 10)
    sleeps = []
    real_sleep = time.sleep
    monkeypatch.setattr(_hipops.time, "sleep", lambda s: sleeps.append(s) or real_sleep(0))
    host = torch.zeros(1, dtype=torch.int32)
    with _HostWords() as words:
        w = words.polled(host, FakeStream())
        threading.Timer(0.02, lambda: host.fill_(2)).start()
        assert words.wait(w).tolist() == [2]
    assert sleeps and set(sleeps) == {0}


# ------------------------------------------------------------------ the eps-deferral policy
def _train_shapes(N, I, r, r0=1, rN=1):
    return [(r0 if mu == 0 else r, I, rN if mu == N - 1 else r) for mu in range(N)]


def _shapes_of_elems(elems):
    """One-core-pair train with exactly ``elems`` swept elements: (1, 1, 1) then (1, elems - 1, 1)."""
    return [(1, 1, 1), (1, elems - 1, 1)]


@pytest.mark.parametrize("mode", ["0", "1", "auto"])
@pytest.mark.parametrize("Bt", [1, 2])
@pytest.mark.parametrize("over", [False, True])
@pytest.mark.parametrize("capped", [True, False])
def test_eps_deferred_policy_table(mode, Bt, over, capped, monkeypatch):
    monkeypatch.setenv("TTR_EPS_DEFERRED", mode)
    limit = _hipops._EPS_DEFERRED_MAX_ELEMS
    shapes = _shapes_of_elems(limit + 1 if over else limit)
    assert _hipops._sweep_elems(shapes) == (limit + 1 if over else limit)
    rmax = [4] if capped else [None]
    want = {"0": False, "1": Bt == 1, "auto": Bt == 1 and not over and capped}[mode]
    assert _hipops._eps_deferred_policy(shapes, Bt, rmax) is want


def test_eps_deferred_policy_reads_the_environment_at_every_call(monkeypatch):
    shapes = _train_shapes(4, 4, 8)
    monkeypatch.setenv("TTR_EPS_DEFERRED", "0")
    assert not _hipops._eps_deferred_policy(shapes, 1, [4, 4, 4])
    monkeypatch.setenv("TTR_EPS_DEFERRED", "auto")
    assert _hipops._eps_deferred_policy(shapes, 1, [4, 4, 4])
    assert not _hipops._eps_deferred_policy(shapes, 1, [4, None, 4])


@pytest.mark.parametrize("N,I,r", [(4, 4, 8), (3, 64, 64)])
def test_both_sweeps_count_the_same_elements(N, I, r, monkeypatch):
    """`_round_tt_sweep_c` hands the policy the cores' own shapes; `_eps_deferred_ok` sees the train after the host loop's L2R
    sweep -- the factor handles (m x n of what each QR factored) and the carry of the last core.  Same number either way, and the
    number the host loop used to compute for itself: carry elements + sum of m n."""
    shapes = _train_shapes(N, I, r)
    facs, k = [], shapes[0][0]
    for r0, Imu, r1 in shapes[:-1]:                      # what the L2R loop leaves: (handle, rows of R before the core, I)
        facs.append((types.SimpleNamespace(m=k * Imu, n=r1), k, Imu))
        k = min(k * Imu, r1)
    last = torch.empty(1, k, shapes[-1][1], shapes[-1][2])
    seen = []
    orig = _hipops._eps_deferred_policy
    monkeypatch.setattr(_hipops, "_eps_deferred_policy", lambda s, Bt, rmax: seen.append((_hipops._sweep_elems(s), Bt)) or orig(s, Bt, rmax))
    monkeypatch.setenv("TTR_EPS_DEFERRED", "auto")
    # (its own answer: the last bond is r x I, and the fused row kernels want rows <= columns)
    assert _hipops._eps_deferred_ok([None] * (N - 1) + [last], facs, [4] * (N - 1)) is (r <= I)
    assert seen == [(_hipops._sweep_elems(shapes), 1)]
    assert seen[0][0] == last.numel() + sum(f.m * f.n for f, _, _ in facs)


def test_eps_deferred_ok_keeps_what_only_the_host_loop_knows(monkeypatch):
    monkeypatch.setenv("TTR_EPS_DEFERRED", "1")
    f = types.SimpleNamespace(m=4, n=8)                  # core 0 = (1, 4, 8): R has 4 rows
    last = torch.empty(1, 4, 4, 1)
    assert _hipops._eps_deferred_ok([None, last], [(f, 1, 4)], [4])                 # bond 1: 4 rows x 4 columns ...
    assert not _hipops._eps_deferred_ok([None, last[:, :, :1]], [(f, 1, 4)], [4])   # ... 4 rows x 1 column
    wide = torch.empty(1, 65, 80, 1)
    assert not _hipops._eps_deferred_ok([None, wide], [(types.SimpleNamespace(m=80, n=65), 1, 80)], [4])   # above 64 rows
    q = _hipops._ExplicitQ(torch.empty(1, 4, 4), torch.empty(1, 4, 8))
    assert not _hipops._eps_deferred_ok([None, last], [(q, 1, 4)], [4])


# ------------------------------------------------------------------ the zero train
@pytest.mark.parametrize("N", [2, 4])
@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_zero_train(N, dt):
    shapes = _train_shapes(N, 5, 7, r0=2, rN=3)
    shapes[1] = (shapes[1][0], 6, shapes[1][2])          # (the mode sizes come from each core)
    out = _hipops._zero_train(shapes, 3, dt, torch.device("cpu"))
    want = [(3, 2 if mu == 0 else 1, shapes[mu][1], 3 if mu == N - 1 else 1) for mu in range(N)]
    assert [tuple(x.shape) for x in out] == want
    assert all(x.dtype == dt and x.device.type == "cpu" and not x.any() for x in out)

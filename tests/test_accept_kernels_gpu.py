"""ttr_accept_count / ttr_accept_expand through the C ABI on a real MI355X, fp32 and fp64 cores, bit for bit against the host mirror.

The inputs are integers (L and the cores in {0, 1, 2}), so every sum is exact in fp64 in any order and the comparison has no
tolerance.  The shapes (automata_cases.KERNEL_SHAPES) put P at 1, 63, 64, 65, 255, 256 and 257 (the wave and the workgroup), r
and r' at 1, 2, 17 and 64 against each other, and I at 1, 2, 3 and 5; further cases: r at ttr_accept_max_rank() and one above it,
every row unproductive, a multiplicity run that crosses the 256 rows of a workgroup of the fill, and the last mode.  Every output
lies in a sentinel-filled buffer with guards; guards and inputs must be unchanged and a second call must give the same bits."""
import functools

import pytest
import torch

import automata_cases as ac
from tntorch_amd import _hip as h
from tntorch_amd import _hostops

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
GUARD = 32
N, MU = 3, 1


class Guarded:
    """n elements of ``dtype`` between two guards of GUARD elements, all filled with ``sentinel``."""

    def __init__(self, n, dtype, sentinel):
        self.n, self.sentinel = n, sentinel
        self.buf = torch.full((GUARD + n + GUARD,), sentinel, dtype=dtype, device="cuda")
        self.ptr = self.buf.data_ptr() + GUARD * self.buf.element_size()

    def read(self):
        """The payload on the CPU, after checking both guards."""
        b = self.buf.cpu()
        assert bool((b[:GUARD] == self.sentinel).all()) and bool((b[GUARD + self.n:] == self.sentinel).all()), "guard overwritten"
        return b[GUARD:GUARD + self.n]


@functools.lru_cache(maxsize=None)
def _mirror(P, r, I, rn, dt, last, zero_rows=None):
    L, core, fiber = ac.kernel_inputs(P, r, I, rn, dt, zero_rows=zero_rows)
    return L, core, fiber, ac.level(_hostops, L, core, fiber, N, MU, last)


def _run(dt, L, core, fiber, m, last):
    """Both entries through the raw C ABI into guarded buffers, twice; everything compared with the mirror's level ``m``."""
    lib = h.lib()
    code = h.dtype_code(dt)
    P, r = L.shape
    I, rn = core.shape[1], core.shape[2]
    K, S = int(m["idx"].numel()), int(m["Xs"].shape[0])
    Ld, cd, fd = L.cuda(), core.cuda(), fiber.cuda()
    firsts = []
    for _ in range(2):
        C = Guarded(P * I, torch.int64, -9)
        assert lib.ttr_accept_count(code, P, r, I, Ld.data_ptr(), fd.data_ptr(), C.ptr, None) == 0, lib.ttr_last_error()
        got = C.read()
        assert torch.equal(got.reshape(P, I), m["C"])
        firsts.append(got)
    assert torch.equal(firsts[0], firsts[1])
    Cd, offd, cntd, idxd = m["C"].cuda(), m["childoff"].cuda(), m["cnt"].cuda(), m["idx"].cuda()
    outs = []
    for _ in range(2):
        Lnew = Guarded(K * rn, torch.float64, -77.0)
        offnew, cntnew = Guarded(K, torch.int64, -9), Guarded(K, torch.int64, -9)
        Xs = Guarded(S * N, torch.int64, -5)
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        rc = lib.ttr_accept_expand(code, P, r, I, rn, K, N, MU, S, Ld.data_ptr(), cd.data_ptr(), Cd.data_ptr(), offd.data_ptr(),
                                   cntd.data_ptr(), idxd.data_ptr(), None if last else Lnew.ptr, offnew.ptr, cntnew.ptr, Xs.ptr,
                                   flag.data_ptr(), None)
        assert rc == 0, lib.ttr_last_error()
        got = (Lnew.read(), offnew.read(), cntnew.read(), Xs.read(), flag.cpu())
        if last:
            assert bool((got[0] == -77.0).all())   # no Lnew is written at the last mode
        else:
            assert torch.equal(got[0].reshape(K, rn), m["Lnew"])
        assert torch.equal(got[1], m["offnew"]) and torch.equal(got[2], m["cntnew"])
        assert torch.equal(got[3].reshape(S, N), m["Xs"])   # column MU filled, the other columns still the sentinel (-5 in both)
        assert int(got[4]) == int(m["flag"]) == 0
        outs.append(got)
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    assert torch.equal(Ld.cpu(), L) and torch.equal(cd.cpu(), core) and torch.equal(fd.cpu(), fiber)
    assert torch.equal(Cd.cpu(), m["C"]) and torch.equal(offd.cpu(), m["childoff"]) and torch.equal(idxd.cpu(), m["idx"])
    # the wrappers: the same level on device tensors
    w = ac.level(h, L, core, fiber, N, MU, last, device="cuda")
    for key in ("C", "offnew", "cntnew", "Xs", "flag"):
        assert w[key].is_cuda and torch.equal(w[key].cpu(), m[key]), key
    assert (w["Lnew"] is None) if last else torch.equal(w["Lnew"].cpu(), m["Lnew"])


def test_rank_limit_is_stated():
    assert h.accept_max_rank() == 1024


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("P, r, I, rn", ac.KERNEL_SHAPES)
def test_count_and_expand(P, r, I, rn, dt):
    zero_rows = tuple(range(0, P, 3)) if P > 2 else None   # every third prefix is unproductive: its children are never listed
    L, core, fiber, m = _mirror(P, r, I, rn, dt, False, zero_rows)
    assert P <= 2 or int(m["idx"].numel()) < P * I
    _run(dt, L, core, fiber, m, False)


@pytest.mark.parametrize("dt", DTYPES)
def test_last_mode_writes_no_left_vectors(dt):
    L, core, fiber, m = _mirror(65, 17, 3, 1, dt, True)
    _run(dt, L, core, fiber, m, True)


@pytest.mark.parametrize("dt", DTYPES)
def test_every_row_unproductive(dt):
    L, core, fiber, m = _mirror(65, 2, 3, 2, dt, False, "all")
    assert m["idx"].numel() == 0 and m["Xs"].shape[0] == 0
    _run(dt, L, core, fiber, m, False)


@pytest.mark.parametrize("dt", DTYPES)
def test_multiplicity_run_crosses_a_block_of_output_rows(dt):
    L = torch.tensor([[300.0], [1.0], [0.0], [700.0]], dtype=torch.float64)
    core = torch.tensor([[[1.0, 2.0], [0.0, 0.0], [1.0, 0.0]]]).to(dt)   # [1, 3, 2]: symbol 1 is never productive
    fiber = core.sum(dim=2)
    m = ac.level(_hostops, L, core, fiber, N, MU, False)
    assert m["cntnew"].tolist() == [900, 300, 3, 1, 2100, 700] and m["Xs"].shape[0] == 4004
    _run(dt, L, core, fiber, m, False)


@pytest.mark.parametrize("dt", DTYPES)
def test_rank_at_the_limit_and_one_above(dt):
    R = h.accept_max_rank()
    L, core, fiber, m = _mirror(3, R, 2, 2, dt, False)
    _run(dt, L, core, fiber, m, False)
    lib, code = h.lib(), h.dtype_code(dt)
    Lb = torch.ones((2, R + 1), dtype=torch.float64, device="cuda")
    fb = torch.ones((R + 1, 2), dtype=dt, device="cuda")
    C = Guarded(4, torch.int64, -9)
    assert lib.ttr_accept_count(code, 2, R + 1, 2, Lb.data_ptr(), fb.data_ptr(), C.ptr, None) == h.E_INVALID
    assert str(R) in lib.ttr_last_error().decode()
    with pytest.raises(ValueError, match=str(R)):
        h.accept_count(Lb, fb)
    assert bool((C.read() == -9).all())
    # expand: r above the limit, and r' above the limit
    for r, rn in ((R + 1, 2), (2, R + 1)):
        Ld = torch.ones((2, r), dtype=torch.float64, device="cuda")
        cd = torch.ones((r, 2, rn), dtype=dt, device="cuda")
        Cd = torch.ones((2, 2), dtype=torch.int64, device="cuda")
        off = torch.tensor([[0, 1], [2, 3]], device="cuda")
        cnt = torch.full((2,), 2, dtype=torch.int64, device="cuda")
        idx = torch.arange(4, device="cuda")
        Xs = torch.full((4, 1), -5, dtype=torch.int64, device="cuda")
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        with pytest.raises(ValueError, match=str(R)):
            h.accept_expand(Ld, cd, Cd, off, cnt, idx, Xs, 0, flag, False)
        assert bool((Xs.cpu() == -5).all()) and int(flag.cpu()) == 0


def test_flag_bits_equal_the_mirror():
    """Negative counts, a sum that differs from the parent's count and an index outside the children: the word equals the mirror's,
    nothing outside the K slots and S rows is written."""
    L, core, fiber = ac.kernel_inputs(4, 3, 2, 2, torch.float64)
    C = _hostops.accept_count(L, fiber)
    cnt = C.sum(1)
    off = torch.cumsum(cnt, 0) - cnt
    childoff = off[:, None] + torch.cumsum(C, 1) - C
    idx = torch.nonzero(C.reshape(-1) > 0).reshape(-1)
    Cneg = C.clone()
    Cneg[0, 0], Cneg[0, 1] = -1, C[0].sum() + 1
    S = int(cnt.sum())
    for Cx, cntx, idxx in ((C, cnt, idx), (Cneg, cnt, idx), (C, cnt + 1, idx), (C, cnt, torch.cat([idx[:-1], torch.tensor([8])])),
                           (C, cnt, torch.cat([idx[:-1], torch.tensor([-1])]))):
        fm = torch.zeros(1, dtype=torch.int32)
        _hostops.accept_expand(L, core, Cx, childoff, cntx, idxx, torch.zeros((S, 1), dtype=torch.int64), 0, fm, False)
        fd = torch.zeros(1, dtype=torch.int32, device="cuda")
        Xs = torch.full((S + 8, 1), -5, dtype=torch.int64, device="cuda")
        h.accept_expand(L.cuda(), core.cuda(), Cx.cuda(), childoff.cuda(), cntx.cuda(), idxx.cuda(), Xs[:S], 0, fd, False)
        assert int(fd.cpu()) == int(fm)
        assert bool((Xs[S:].cpu() == -5).all())

"""Pass-through items of the two-pass truncation without the identity round trip (TTR_KNOB_FLAT_PASS = 1: ttr_eigh_trunc_pass does
not write V = I for an item whose kept spectrum is flat, ttr_project_flat takes U = V1[:, :ro] and 1 / sigma from pass 1's sigma for
it) against the round trip (0): the same bits -- new core, left = U sigma, info and sigma -- at the kernel level, on both sides of
the lean instances' threshold, through ttr_round_tt and through the host loop, in eps mode and in fp64.  V and sigma of pass 2 are
preset to NaN here: a flat item's V stays NaN under knob 1 (not written), and no NaN reaches a result (not read)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

R = 64
THR = 0.125   # the sweep's flat-spectrum threshold (_hipops.FLAT_SPECTRUM_THR)


def _hip():
    from tntorch_amd import _hip

    _hip.lib()
    return _hip


def _both(h, fn):
    """fn() under knob 1 (first: nothing of knob 0's identity is left in a reused allocation) and knob 0."""
    out = {}
    try:
        for v in (1, 0):
            h.set_knob(h.KNOB_FLAT_PASS, v)
            out[v] = fn()
    finally:
        h.set_knob(h.KNOB_FLAT_PASS, 1)
    return out[1], out[0]


# ------------------------------------------------------------------ kernel level
@functools.lru_cache(maxsize=None)
def _factors(B, n, seed):
    """Orthogonal factors (float64, CPU): Q32 [B, 32, 32], Q64 [B, 64, 64], P [B, n, 64] with orthonormal columns."""
    g = torch.Generator().manual_seed(seed)
    Q64 = torch.linalg.qr(torch.randn(8, 64, 64, generator=g, dtype=torch.float64))[0]
    Q32 = torch.linalg.qr(torch.randn(8, 32, 32, generator=g, dtype=torch.float64))[0]
    P = torch.linalg.qr(torch.randn(8, n, 64, generator=g, dtype=torch.float64))[0]
    idx = torch.arange(B) % 8
    return Q32[idx], Q64[idx], P[idx]


FLAT = "flat"       # kept singular values within a factor 8 of each other, no close pair
DECAY = "decay"     # sigma_j = 2^-j: the kept ones reach far below sigma_0 / 8
ZERO = "zero"


def _matrices(kinds, rows32, n, dt, seed=7, scale=None):
    """M [B, 64, n] = Q diag(s) P^T with the spectrum `kinds[b]` names; rows32[b] != 0: rank 32, rows 32.. exactly zero."""
    B = len(kinds)
    Q32, Q64, P = _factors(B, n, seed)
    M = torch.zeros(B, R, n, dtype=torch.float64)
    for b, kind in enumerate(kinds):
        k = 32 if rows32[b] else 64
        j = torch.arange(k, dtype=torch.float64)
        s = {FLAT: 1.0 - 0.4 * j / k, DECAY: 2.0 ** (-j), ZERO: 0.0 * j}[kind]
        Q = Q32[b] if rows32[b] else Q64[b]
        M[b, :k] = (Q * s) @ P[b, :, :k].T
        if scale is not None:
            M[b] *= scale[b]
    return M.to(dt).cuda()


def _pass2(h, G2, cap, flat, sig1):
    """ttr_eigh_trunc_pass (batch mode, live-prefix Jacobi) into V and sigma preset to NaN -> (V, sigma, info)."""
    B, parts, n, _ = G2.shape
    dt = h.dtype_code(G2.dtype)
    V = torch.full((B, n, n), float("nan"), dtype=G2.dtype, device="cuda")
    sig = torch.full((B, n), float("nan"), dtype=G2.dtype, device="cuda")
    info = torch.full((B,), -5, dtype=torch.int32, device="cuda")
    wsb = h.lib().ttr_eigh_workspace_bytes(dt, n, B)
    ws = h._workspace(wsb, G2.device)
    h._call("ttr_eigh_trunc_pass", dt, n, B, G2.data_ptr(), n, parts * n * n, parts, n * n, V.data_ptr(), n, n * n, sig.data_ptr(), n,
            info.data_ptr(), h.EIG_RAW, 0, 0.0, None, int(cap), h.SOLVER_JACOBI_LIVE, None, h._ptr(flat), h._ptr(sig1), n,
            h._ptr(ws), wsb)
    return V, sig, info


def _bond(h, M, rows32, cap):
    """One bond of the batch-mode sweep on the carry M, kernel by kernel as _hipops._truncate_rows64 / ttr_round_tt enqueue them
    -> (right, left, info, sigma, V of pass 2, flat)."""
    G = h.rowgram(M, rows32=rows32)
    V1, sig1, _, flat = h.eigh_top(G, cap, THR)
    G2 = h.rowgram(M, V1, skip=flat, rows32=rows32)
    V, sig, info = _pass2(h, G2, cap, flat, sig1)
    right, left = h.project(M, V1, V, sig, cap, scale_right=True, rows32=rows32, flat=flat, sigma1=sig1)
    return right, left, info, sig, V, flat


def _check_bond(h, M, rows32, cap, want_flat=None):
    (r1, l1, i1, s1, V1k, f1), (r0, l0, i0, s0, V0k, f0) = _both(h, lambda: _bond(h, M, rows32, cap))
    assert torch.equal(f1, f0)
    fl = f1 != 0
    if want_flat is not None:   # the batch is what the case says it is
        assert fl.tolist() == want_flat, fl.tolist()
    assert torch.equal(r1, r0) and torch.equal(l1, l0) and torch.equal(i1, i0) and torch.equal(s1, s0)
    assert not torch.isnan(r1).any() and not torch.isnan(l1).any() and not torch.isnan(s1).any()
    if fl.any():   # knob 1 left V alone, knob 0 wrote the identity
        assert torch.isnan(V1k[fl]).all()
        assert torch.equal(V0k[fl], torch.eye(R, dtype=M.dtype, device="cuda").expand(int(fl.sum()), R, R))
    if (~fl).any():
        assert torch.equal(V1k[~fl], V0k[~fl])
    return fl


BATCHES = {
    "all flat": ([FLAT] * 5, [True] * 5),
    "none flat": ([DECAY] * 5, [False] * 5),
    "mixed": ([FLAT, DECAY, FLAT, DECAY, FLAT], [True, False, True, False, True]),
}


@pytest.mark.parametrize("cap", [32, 8])
@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("n", [64, 128])
@pytest.mark.parametrize("batch", list(BATCHES))
def test_project_after_the_eigensolvers(batch, n, packed, cap):
    """Batches of 5 (the generic projection): all flat, none flat, flat items at 0, 2 and 4; with and without `rows32`; kept rank 32
    and a cap of 8; the last bond's shape (n = 64) and n = 128."""
    h = _hip()
    kinds, want = BATCHES[batch]
    flags = [1 if packed else 0] * 5
    M = _matrices(tuple(kinds), tuple(flags), n, torch.float32)
    rows32 = torch.tensor(flags, dtype=torch.int32, device="cuda") if packed else None
    _check_bond(h, M, rows32, cap, want)


@pytest.mark.parametrize("packed", [True, False])
def test_zero_and_scaled_items(packed):
    """An all-zero item (sigma_0 = 0: never flat; 1 / sigma counts as 0 either way) and items scaled by 2^40 beside plain ones."""
    h = _hip()
    kinds = [FLAT, ZERO, FLAT, DECAY, ZERO]
    scale = [2.0 ** 40, 1.0, 1.0, 2.0 ** 40, 1.0]
    flags = [1 if packed else 0] * 5
    M = _matrices(tuple(kinds), tuple(flags), 128, torch.float32, scale=tuple(scale))
    rows32 = torch.tensor(flags, dtype=torch.int32, device="cuda") if packed else None
    for cap in (32, 8):
        fl = _check_bond(h, M, rows32, cap)
        assert fl.tolist()[0] and fl.tolist()[2] and not fl.tolist()[1] and not fl.tolist()[3] and not fl.tolist()[4]


@pytest.mark.parametrize("B", [256, 257])
def test_lean_instance_threshold(B):
    """256 and 257 items (the threshold of the lean `rows32` launches): flat `rows32` items on the lean instance, one non-flat
    `rows32` item beside them, and one item without the flag on the generic instance's second launch (the returning twin)."""
    h = _hip()
    kinds, flags = [FLAT] * B, [1] * B
    kinds[3] = DECAY
    flags[7] = 0
    M = _matrices(tuple(kinds), tuple(flags), 64, torch.float32)
    rows32 = torch.tensor(flags, dtype=torch.int32, device="cuda")
    want = [True] * B
    want[3] = False
    _check_bond(h, M, rows32, 32, want)


def test_fp64_flat_batch():
    """fp64: the generic projection and the same pass-through branch of the Jacobi kernel."""
    h = _hip()
    M = _matrices((FLAT,) * 4, (1, 0, 1, 0), 128, torch.float64)
    rows32 = torch.tensor([1, 0, 1, 0], dtype=torch.int32, device="cuda")
    _check_bond(h, M, rows32, 32, [True] * 4)


def test_null_operands_are_the_old_entry():
    """ttr_project_flat without `flat`, and with `flat` but without V1, is ttr_project."""
    h = _hip()
    B, n, cap = 5, 128, 32
    M = _matrices((FLAT, DECAY, FLAT, DECAY, FLAT), (1,) * 5, n, torch.float32)
    rows32 = torch.ones(B, dtype=torch.int32, device="cuda")
    G = h.rowgram(M, rows32=rows32)
    V1, sig1, _, flat = h.eigh_top(G, cap, THR)
    V, sig, _ = h.eigh_trunc(h.rowgram(M, V1, skip=flat, rows32=rows32), h.EIG_RAW, False, 0.0, cap, abs_floor=h.SOLVER_JACOBI_LIVE,
                             skip_items=flat, sigma_in=sig1)

    def old(v1):
        right = torch.empty((B, cap, n), dtype=M.dtype, device="cuda")
        left = torch.empty((B, R, cap), dtype=M.dtype, device="cuda")
        h._call("ttr_project", h.dtype_code(M.dtype), R, n, cap, B, M.data_ptr(), n, R * n, h._ptr(v1), R, R * R, V.data_ptr(), R, R * R,
                sig.data_ptr(), R, 1, right.data_ptr(), n, cap * n, left.data_ptr(), cap, R * cap, rows32.data_ptr())
        return right, left

    assert flat.bool().tolist() == [True, False, True, False, True]
    for v1, fl in ((V1, None), (None, flat)):
        r_new, l_new = h.project(M, v1, V, sig, cap, scale_right=True, rows32=rows32, flat=fl, sigma1=sig1 if fl is not None else None)
        r_old, l_old = old(v1)
        assert torch.equal(r_new, r_old) and torch.equal(l_new, l_old)


# ------------------------------------------------------------------ sweep level
def _gg(B, seed, decaying=()):
    """B four-core trains 64^4 on the device: g + g with g of rank 32 (every large bond flat, rows packed); the items of `decaying`
    are rank-64 trains with bond singular values ~ 2^-j instead."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    ranks = [1, 32, 32, 32, 1]
    cores = []
    for k in range(4):
        r0, r1 = ranks[k], ranks[k + 1]
        a = torch.randn(B, r0, 64, r1, generator=g, device="cuda") / 8.0
        c = torch.zeros(B, 1 if k == 0 else 64, 64, 1 if k == 3 else 64, device="cuda")
        if k == 0:
            c[:, :, :, :32] = a
            c[:, :, :, 32:] = a
        elif k == 3:
            c[:, :32] = a
            c[:, 32:] = a
        else:
            c[:, :32, :, :32] = a
            c[:, 32:, :, 32:] = a
        for b in decaying:
            d = torch.randn(c.shape[1:], generator=g, device="cuda") / (c.shape[1] * 64) ** 0.5
            if k < 3:
                d = d * 2.0 ** (-torch.arange(64, device="cuda", dtype=torch.float32))
            c[b] = d
        cores.append(c)
    return cores


def _four_ways(monkeypatch, make, call):
    """call(make()) through ttr_round_tt and through the host loop, under both knob values -> {(sweep_c, knob): cores}."""
    from tntorch_amd import _hipops

    h = _hip()
    out = {}
    for sweep_c in (True, False):
        monkeypatch.setattr(_hipops, "SWEEP_C_ENABLED", sweep_c)
        n0 = _hipops.SWEEP_C_CALLS

        def run():
            t = make()
            call(t)
            return [c.clone() for c in t.cores]

        out[sweep_c, 1], out[sweep_c, 0] = _both(h, run)
        assert (_hipops.SWEEP_C_CALLS - n0 >= 2) == sweep_c and (sweep_c or _hipops.SWEEP_C_CALLS == n0)   # both runs, or neither
    return out


def _all_equal(out):
    ref = out[True, 1]
    for key, cores in out.items():
        assert len(cores) == len(ref) and all(torch.equal(a, b) for a, b in zip(cores, ref)), key
    assert not any(torch.isnan(c).any() for c in ref)


@pytest.mark.parametrize("B,decaying", [(256, ()), (6, (1, 4))])
def test_round_tt_batch(B, decaying, monkeypatch):
    """round_tt(rmax=32) of 256 trains g + g (the lean instances, every item flat on every large bond) and of 6 with two
    decaying-spectrum items among them: ttr_round_tt and the host loop, knob 1 and 0 -- four results, one set of bits."""
    import tntorch_amd as tn

    cores = _gg(B, seed=11 + B, decaying=decaying)
    out = _four_ways(monkeypatch, lambda: tn.Tensor([c.clone() for c in cores], batch=True), lambda t: t.round_tt(rmax=32))
    _all_equal(out)
    assert [c.shape[-1] for c in out[True, 1]] == [32, 32, 32, 1]


def test_round_tt_eps_mode(monkeypatch):
    """One train, eps = 1e-4 under a cap of 32, ranks kept on the device: the certified flat test on the `rows32` items decides which
    items pass through.  Selected ranks (read back from ranks_dev) and cores, four ways."""
    import tntorch_amd as tn

    monkeypatch.setenv("TTR_EPS_DEFERRED", "1")
    cores = [c[0] for c in _gg(1, seed=3)]
    ranks = []

    def call(t):
        t.round_tt(eps=1e-4, rmax=32)
        ranks.append(list(t.ranks_tt))

    out = _four_ways(monkeypatch, lambda: tn.Tensor([c.clone() for c in cores]), call)
    _all_equal(out)
    assert len(ranks) == 4 and all(r == [1, 32, 32, 32, 1] for r in ranks), ranks

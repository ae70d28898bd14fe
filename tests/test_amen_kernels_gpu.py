"""``ttr_cg_dot``, ``ttr_cg_update`` and ``ttr_cg_direction`` through the binding ``_hip``, on the device, in fp32 and fp64: each
launch alone against an evaluation of its own inputs in extended precision on the CPU (the bounds of ``amen_cases``), the bits
from aligned pointers against those from pointers offset by an element, the steps that must write nothing, and the solve built
on them (``_hipops.cg_solve``) against ``ttsolve._cg`` in fp64."""
import pytest
import torch

import amen_cases as ac
import solve_cases as sc
from tntorch_amd import _hostops, ttsolve

pytestmark = pytest.mark.gpu

DTYPES = sc.DTYPES


def hip():
    from tntorch_amd import _hip

    return _hip


def on_device(vs, offset=0):
    """Device copies of CPU vectors; ``offset`` elements in front of each, so that the views start off a 16-byte boundary."""
    out = []
    for v in vs:
        buf = torch.zeros(v.numel() + offset, dtype=v.dtype, device="cuda")
        buf[offset:] = v.cuda()
        out.append(buf[offset:])
    return out


def one_step(n, dt, step, rs, thr2, offset=0, pBp=None, seed=0, bad=0.0):
    """dot, update, direction on fresh device copies of the vectors of (n, dt, seed); every launch is checked alone against the
    snapshots around it.  ``pBp``: row 0 of ``part`` is replaced by shares of this value before the update.  Returns the final
    snapshot and whether the step was live."""
    H = hip()
    p, Bp, v, r = on_device(ac.vectors(n, dt, seed), offset)
    assert (p.data_ptr() % 16 != 0) == (offset % ac.pack(dt) != 0)
    parts = H.cg_parts(dt, n)
    part = torch.full((2, parts), float("nan"), dtype=torch.float64, device="cuda")
    state = ac.make_state(rs, thr2, step & 1, bad).cuda()
    H.cg_dot(p, Bp, part)
    s0 = ac.snapshot(p=p, Bp=Bp, v=v, r=r, part=part, state=state)
    ac.check_dot(s0["p"], s0["Bp"], s0["part"])
    if pBp is not None:
        part[0].copy_(ac.spread(pBp, parts).cuda())
        s0 = ac.snapshot(p=p, Bp=Bp, v=v, r=r, part=part, state=state)
    H.cg_update(step, p, Bp, v, r, part, state)
    s1 = ac.snapshot(p=p, Bp=Bp, v=v, r=r, part=part, state=state)
    live = ac.check_update(step, s0, s1)
    H.cg_direction(step, r, p, part, state)
    s2 = ac.snapshot(p=p, Bp=Bp, v=v, r=r, part=part, state=state)
    ac.check_direction(step, s1, s2)
    return s2, live


@pytest.mark.parametrize("dt", DTYPES)
def test_each_launch_at_every_size(dt):
    """Pack edges, the block of 256 packs, one, two and three workgroups; both parities of the step."""
    H = hip()
    sizes = ac.kernel_sizes(dt)
    assert [H.cg_parts(dt, n) for n in sizes[-3:]] == [1, 2, 3]
    for i, n in enumerate(sizes):
        assert H.cg_workspace_bytes(dt, n) == 16 * H.cg_parts(dt, n)
        _, live = one_step(n, dt, i & 1, rs=0.75, thr2=1e-3, pBp=1.5)      # alpha = 0.5
        assert live


@pytest.mark.parametrize("dt", DTYPES)
def test_offset_views_give_the_same_bits(dt):
    """Every vector as a view offset by one element takes the element loads: the same bits as the 16-byte packs."""
    for n in ac.kernel_sizes(dt)[2:]:
        a, _ = one_step(n, dt, 0, rs=0.75, thr2=1e-3, pBp=1.5)
        b, _ = one_step(n, dt, 0, rs=0.75, thr2=1e-3, pBp=1.5, offset=1)
        for k in ("p", "v", "r", "part", "state"):
            assert torch.equal(a[k], b[k]), (n, k)
    # and the sums of the dot launch itself (row 0 is not replaced)
    n = ac.kernel_sizes(dt)[-1]
    a, _ = one_step(n, dt, 1, rs=0.75, thr2=1e-3)
    b, _ = one_step(n, dt, 1, rs=0.75, thr2=1e-3, offset=1)
    assert all(torch.equal(a[k], b[k]) for k in ("p", "v", "r", "part", "state"))


@pytest.mark.parametrize("dt", DTYPES)
def test_steps_that_are_not_live_write_no_vector(dt):
    """Frozen (rs <= thr2), p^T B p < 0 and p^T B p == 0 exactly: v, r and p keep their bits (check_update / check_direction
    assert it), and the count rises by one per such step only when rs > thr2."""
    for n in (ac.pack(dt) + 1, ac.kernel_sizes(dt)[-2]):
        for rs, thr2, pBp, bump in ((1.0, 2.0, 3.0, 0), (1.0, 1.0, 3.0, 0), (1.0, 2.0, -3.0, 0), (2.0, 1.0, -3.0, 1), (2.0, 1.0, 0.0, 1)):
            for step in (0, 1):
                s, live = one_step(n, dt, step, rs, thr2, pBp=pBp, bad=4.0)
                assert not live and float(s["state"][3]) == 4.0 + bump and float(s["state"][1 - (step & 1)]) == rs


@pytest.mark.parametrize("dt", DTYPES)
def test_zero_right_hand_side(dt):
    """f == 0: thr2 == 0 and rs == 0, p = r = 0.  Nothing becomes NaN or Inf."""
    H = hip()
    n = 2 * ac.pack(dt) + 1
    p, Bp, v, r = (torch.zeros(n, dtype=dt, device="cuda") for _ in range(4))
    part = torch.zeros((2, H.cg_parts(dt, n)), dtype=torch.float64, device="cuda")
    state = torch.zeros(8, dtype=torch.float64, device="cuda")
    for step in range(3):
        H.cg_dot(p, Bp, part)
        H.cg_update(step, p, Bp, v, r, part, state)
        H.cg_direction(step, r, p, part, state)
    for t in (p, Bp, v, r, part, state):
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) == 0.0


@pytest.mark.parametrize("dt", DTYPES)
def test_the_same_call_twice_gives_the_same_bits(dt):
    n = ac.kernel_sizes(dt)[-1]
    a, _ = one_step(n, dt, 0, rs=0.75, thr2=1e-3)
    b, _ = one_step(n, dt, 0, rs=0.75, thr2=1e-3)
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("dt", DTYPES)
def test_cg_solve_against_cg(dt):
    """Ten steps of ``_hipops.cg_solve`` on a local problem of the laplace system at ranks (3, 4), against ``ttsolve._cg`` on fp64
    CPU copies of the same operands: ||v - v_ref|| <= 10 cond u ||v_ref||, and stat to the same."""
    from tntorch_amd import _hipops

    Phi, A1, Psi, f, x0, cond = ac.local_problem(dt)
    stat = torch.zeros(2, dtype=dt, device="cuda")
    keep = x0.clone()
    x0d = x0.cuda()
    v = _hipops.cg_solve(Phi.cuda(), A1.cuda(), Psi.cuda(), f.cuda(), x0d, 0.0, 10, stat)
    assert torch.equal(x0d.cpu(), keep) and v.shape == f.shape and v.dtype == dt
    stat64 = torch.zeros(2, dtype=torch.float64)
    ref = ttsolve._cg(_hostops, Phi.double(), A1.double(), Psi.double(), f.double(), x0.double(), 0.0, 10, stat64)
    bound = 10 * cond * sc.unit(dt)
    err = float((v.cpu().double() - ref).norm() / ref.norm())
    print("cg_solve {}: ||v - _cg|| / ||v|| = {:.3e} (bound {:.3e}); stat {} against {}".format(dt, err, bound, stat.tolist(), stat64.tolist()))
    assert err <= bound
    assert abs(float(stat[0]) - float(stat64[0])) <= bound * float(stat64[0]) and float(stat[1]) == float(stat64[1]) == 0.0
    # an indefinite local problem is counted, not solved
    stat.zero_()
    _hipops.cg_solve(Phi.cuda(), -A1.cuda(), Psi.cuda(), f.cuda(), x0d, 0.0, 3, stat)
    assert float(stat[1]) >= 1.0


def test_cabi_refusals_without_a_launch():
    """Bad dtype, n = 0, a null pointer and a short workspace return their codes; the pointers are valid device buffers of the
    stated sizes, and ``part`` is larger than the workspace it is said to be."""
    H = hip()
    L = H.lib()
    n = 8
    p, Bp, v, r = (torch.ones(n, dtype=torch.float32, device="cuda") for _ in range(4))
    part = torch.zeros((2, 4), dtype=torch.float64, device="cuda")
    state = ac.make_state(1.0, 0.0, 0).cuda()
    torch.cuda.synchronize()
    P, BP, X, R, PART, STATE = (t.data_ptr() for t in (p, Bp, v, r, part, state))
    calls = {
        "ttr_cg_dot": lambda dtype=0, n=n, a=P, part=PART, wsb=16: L.ttr_cg_dot(dtype, n, a, BP, part, wsb, None),
        "ttr_cg_update": lambda dtype=0, n=n, a=P, part=PART, wsb=16: L.ttr_cg_update(dtype, 0, n, a, BP, X, R, part, wsb, STATE, None),
        "ttr_cg_direction": lambda dtype=0, n=n, a=P, part=PART, wsb=16: L.ttr_cg_direction(dtype, 0, n, R, a, part, wsb, STATE, None),
    }
    for name, call in calls.items():
        for kw, code, text in ((dict(dtype=7), H.E_INVALID, "bad dtype 7"), (dict(n=0), H.E_INVALID, "n = 0 < 1"),
                               (dict(a=None), H.E_INVALID, "null pointer"), (dict(part=None), H.E_INVALID, "null pointer"),
                               (dict(wsb=8), H.E_WORKSPACE, "workspace of 8 bytes, 16 needed")):
            assert call(**kw) == code and name in L.ttr_last_error().decode() and text in L.ttr_last_error().decode()
    assert L.ttr_cg_update(0, 0, n, P, BP, P, R, PART, 16, STATE, None) == H.E_INVALID and "overlap" in L.ttr_last_error().decode()
    assert L.ttr_cg_parts(7, 5) == H.E_INVALID and L.ttr_cg_workspace_bytes(0, 0) == H.E_INVALID
    torch.cuda.synchronize()
    assert float(p.sum() + Bp.sum() + v.sum() + r.sum()) == 4.0 * n and float(part.abs().max()) == 0.0
    assert torch.equal(state.cpu(), ac.make_state(1.0, 0.0, 0))

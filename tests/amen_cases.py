"""What the tests of ``tn.tt_amen_solve``, of the mirror of its CG step (``_hostops.cg_dot`` / ``cg_update`` / ``cg_direction``) and
of the kernels behind it (``ttr_cg_dot`` / ``ttr_cg_update`` / ``ttr_cg_direction``) share.  The systems are those of
``solve_cases``; every truth of a solve is dense fp64 and independent of the package.

The bounds of one launch, each checked against an evaluation of the SAME inputs in extended precision (numpy longdouble, 64
bits of mantissa on x86; ``math.fsum`` of the products where longdouble is no wider than double), u = ``solve_cases.unit``:
  a sum of n products      |s - sum a_i b_i| <= n 2^-53 sum |a_i||b_i|: every chain of fmas and every tree of partial sums over n
                           terms stays below gamma_n of the sum of the magnitudes (Higham, section 3.1), in double
  a vector update          |y - (a + c b)| <= 2 u (|a| + |c||b|): one rounding of the product and one of the sum in the mirror
                           (the kernel's fma has one), and in fp32 the second rounding of the fp64 value, 2^-29 of it
  alpha, beta              quotients of two doubles: equal to the double quotient within 2 units of 2^-53
  the sum of the partials  added in the order of their rows in double: the same double, exactly
"""
import math

import numpy as np
import torch

import solve_cases as sc

KICKS = (1, 2, 4)
SYSTEMS = [(name, rhs) for name in sc.MATRICES for rhs in ("random", "product")]
_WIDE = np.finfo(np.longdouble).nmant >= 63


def residual_bound(cond, tol):
    """The stop gives ``tol``; the final rounding at ``tol / 10`` perturbs x by that much of ||x||, b by ``cond`` times it."""
    return (1 + cond / 10) * tol


def check_solution(name, rhs, kick, x, info, D, bd, cond, tol):
    res = sc.rel_residual(D, bd, x)
    ranks = [int(r) for r in x.ranks_tt][1:-1]
    print("amen {} {} kickrank {}: {} sweeps, dense residual {:.3e} (bound {:.3e}), info {:.3e}, ranks {} from {}".format(
        name, rhs, kick, info["sweeps"], res, residual_bound(cond, tol), info["residual"], ranks, info["ranks"][-1]))
    assert info["converged"] and info["sweeps"] == len(info["local_residuals"]) == len(info["ranks"])
    assert res <= residual_bound(cond, tol)
    assert all(r <= full for r, full in zip(ranks, sc.FULL_RANKS[name]))
    if rhs == "product":
        assert all(r <= 2 + kick for r in ranks)
    return res


# ------------------------------------------------------------------ one CG step, launch by launch
def pack(dt):
    return 4 if dt == torch.float32 else 2


def kernel_sizes(dt):
    """Pack edges, the block of 256 packs, the smallest n with two workgroups (a further one joins per 1024 packs), that n minus
    one, and one n with three."""
    V = pack(dt)
    two = 1024 * V + 1
    return [1, V - 1, V, V + 1, 256 * V - 1, 256 * V, 256 * V + 1, two - 1, two, 2 * 1024 * V + 5]


def vectors(n, dt, seed=0, count=4):
    g = torch.Generator().manual_seed(1000 * seed + n)
    return [torch.randn(n, dtype=torch.float64, generator=g).to(dt) for _ in range(count)]


def _ld(t):
    return np.asarray(t.detach().double().cpu().numpy(), dtype=np.longdouble)


def dot_ref(a, b):
    """(sum a_i b_i in extended precision, the bound n 2^-53 sum |a_i||b_i|)."""
    x, y = _ld(a), _ld(b)
    ref = float((x * y).sum()) if _WIDE else math.fsum((x * y).tolist())
    return ref, a.numel() * 2.0 ** -53 * float((np.abs(x) * np.abs(y)).sum())


def seq_sum(row):
    s = float(row[0])
    for v in row[1:].tolist():
        s += float(v)
    return s


def make_state(rs, thr2, slot, bad=0.0):
    """fp64[8]: rs in ``slot``, a poison in the other slot and in the words a launch overwrites."""
    st = torch.full((8,), -7.5, dtype=torch.float64)
    st[slot], st[2], st[3] = rs, thr2, bad
    return st


def spread(total, parts, seed=3):
    """``parts`` doubles whose sum in increasing order is what a launch finishes: random shares of ``total``."""
    g = torch.Generator().manual_seed(seed + parts)
    w = torch.rand(parts, dtype=torch.float64, generator=g) + 0.5
    return total * w / w.sum()


def snapshot(**tensors):
    return {k: v.detach().cpu().clone() for k, v in tensors.items()}


def _close(got, want):
    return abs(got - want) <= 2 * 2.0 ** -53 * abs(want)


def check_dot(p, Bp, part):
    ref, bound = dot_ref(p, Bp)
    got = seq_sum(part[0])
    print("cg_dot n = {}: error / bound = {:.3f}".format(p.numel(), abs(got - ref) / max(bound, 1e-300)))
    assert abs(got - ref) <= bound
    return got


def check_update(step, before, after):
    """``before`` / ``after``: snapshots of p, Bp, v, r, part [2, parts], state around one cg_update.  Returns live."""
    slot, dt, n = step & 1, before["v"].dtype, before["v"].numel()
    s0, s1 = before["state"], after["state"]
    pBp = seq_sum(before["part"][0])
    rs, thr2 = float(s0[slot]), float(s0[2])
    active, good = rs > thr2, pBp > 0
    live = active and good
    assert float(s1[4]) == (1.0 if live else 0.0) and float(s1[6]) == pBp
    assert float(s1[3]) == float(s0[3]) + (1.0 if active and not good else 0.0)
    alpha = float(s1[5])
    assert _close(alpha, rs / pBp) if live else alpha == 0.0
    assert torch.equal(s1[:3], s0[:3]) and torch.equal(s1[7:], s0[7:])
    assert torch.equal(after["p"], before["p"]) and torch.equal(after["Bp"], before["Bp"])
    assert torch.equal(after["part"][0], before["part"][0])
    if not live:
        assert torch.equal(after["v"], before["v"]) and torch.equal(after["r"], before["r"])
        assert float(after["part"][1].abs().max()) == 0.0
        return False
    u = sc.unit(dt)
    for name, sign, d in (("v", 1.0, "p"), ("r", -1.0, "Bp")):
        ref = _ld(before[name]) + np.longdouble(sign * alpha) * _ld(before[d])
        bound = 2 * u * (np.abs(_ld(before[name])) + abs(alpha) * np.abs(_ld(before[d])))
        err = np.abs(_ld(after[name]) - ref)
        print("cg_update {} n = {}: largest error / bound = {:.3f}".format(name, n, float((err / np.maximum(bound, 1e-300)).max())))
        assert bool((err <= bound).all()), name
    ref, bound = dot_ref(after["r"], after["r"])
    got = seq_sum(after["part"][1])
    assert abs(got - ref) <= bound
    return True


def check_direction(step, before, after):
    """Snapshots of r, p, part, state around one cg_direction (state[4] says whether the update was live)."""
    slot, dt, n = step & 1, before["p"].dtype, before["p"].numel()
    s0, s1 = before["state"], after["state"]
    live = float(s0[4]) != 0.0
    rs, rsn = float(s0[slot]), seq_sum(before["part"][1])
    beta = float(s1[7])
    keep = [i for i in range(7) if i != 1 - slot]
    assert torch.equal(s1[keep], s0[keep]) and torch.equal(after["r"], before["r"]) and torch.equal(after["part"], before["part"])
    if not live:
        assert beta == 0.0 and float(s1[1 - slot]) == rs and torch.equal(after["p"], before["p"])
        return
    assert float(s1[1 - slot]) == rsn and _close(beta, rsn / max(rs, float(torch.finfo(dt).tiny)))
    ref = _ld(before["r"]) + np.longdouble(beta) * _ld(before["p"])
    bound = 2 * sc.unit(dt) * (np.abs(_ld(before["r"])) + abs(beta) * np.abs(_ld(before["p"])))
    err = np.abs(_ld(after["p"]) - ref)
    print("cg_direction n = {}: largest error / bound = {:.3f}".format(n, float((err / np.maximum(bound, 1e-300)).max())))
    assert bool((err <= bound).all())


# ------------------------------------------------------------------ a local problem of the laplace system
def local_problem(dt, ranks=(3, 4), seed=7):
    """(Phi, A_1, Psi, f, x0, cond) of site 1 of the ``laplace`` system for a random train of these ranks orthogonalised towards the
    site, CPU tensors of ``dt``: B = (Phi, A_1, Psi) is a projection of the matrix, so its condition number is at most the matrix's."""
    from tntorch_amd import _hostops

    cores, dims, _, cond = sc.matrix("laplace")
    xs = [c[None] for c in sc.train_cores(dims, list(ranks), seed)]
    _hostops.left_orthogonalize(xs, 0)
    _hostops.right_orthogonalize(xs, 2)
    one = torch.ones((1, 1, 1), dtype=torch.float64)
    Phi = _hostops.env_update("left", one, cores[0], xs[0][0], xs[0][0])
    Psi = _hostops.env_update("right", one, cores[2], xs[2][0], xs[2][0])
    g = torch.Generator().manual_seed(seed + 1)
    f, x0 = (torch.randn((ranks[0], dims[1], ranks[1]), dtype=torch.float64, generator=g) for _ in range(2))
    return Phi.to(dt), cores[1].to(dt), Psi.to(dt), f.to(dt), x0.to(dt), cond

"""``tn.tt_amen_solve`` and its kernels ``ttr_cg_dot`` / ``ttr_cg_update`` / ``ttr_cg_direction`` on one MI355X.  Reads nothing but
this package.

    python tools/amen_bench.py                      # every row
    python tools/amen_bench.py --only step --reps 20
    python tools/amen_bench.py --only whole

Step rows (``kind: step``): one conjugate-gradient step on vectors of n = R I R elements, R in {16, 32, 64}, I = 64, fp32 and
fp64, for the SPD local operator 2 I + 0.25 L (identity interfaces around the middle core of the Laplace TT-matrix):
  cg              ``_hipops.cg_dot`` + ``cg_update`` + ``cg_direction`` (3 launches)
  cg_torch        the host mirror's code (``_hostops.cg_dot`` / ``cg_update`` / ``cg_direction``) on device tensors
  step            the matvec ``_hipops.local_matvec`` (2 launches) and ``cg``
  step_torch      the same matvec and ``cg_torch``
  dot, update, direction   each kernel alone; ``update_frozen``: the update with thr2 above rs, which sums the partials and leaves
A timed window is ``inner`` consecutive steps between device events from the same restored vectors and state, the variants
alternate inside the repetition loop, and the figure is the median over --reps of window / inner.  ``gbytes_per_s``: 2 n
elements read by the dot, 4 n read and 2 n written by the update, 2 n read and n written by the direction.

Whole rows (``kind: whole``): ``tn.tt_amen_solve`` (defaults: kickrank 2, tol sqrt(eps), nswp 20, local_iters 50) of
I + 0.25 sum_k L_k, L = tridiag(-1, 2, -1), on [64]^8 and [16]^6 with a random rank-2 right-hand side, from the rank-1 start,
fp32 and fp64 (median of --whole-reps, alternating):
  tt_amen_solve   as a user calls it
  cg_torch        the same driver with ``ttsolve._cg`` on device tensors as the local solver (the matvec stays ``local_matvec``)
  tt_solve        ``tn.tt_solve`` with the same tol from a random start at the ranks ``tt_amen_solve`` ended with
One JSON line per row, appended to profiles/amen_bench_mi355x.jsonl (``--out``: another file).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "amen_bench_mi355x.jsonl")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def alternate(fns, reps, before=None):
    """Median ms of every variant, the variants taking turns inside each repetition (``before`` runs untimed ahead of each
    window); and the last result of each."""
    ts, last = {k: [] for k in fns}, {}
    for fn in fns.values():
        if before:
            before()
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in fns.items():
            if before:
                before()
            ms, last[k] = timed(fn)
            ts[k].append(ms)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ts.items()}, last


def emit(line):
    print(json.dumps(line), flush=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(line) + "\n")


def laplace_cores(dims, dt, dev, c=0.25):
    cores = []
    for k, n in enumerate(dims):
        I = torch.eye(n, dtype=torch.float64)
        L = c * (2 * I - torch.diag(torch.ones(n - 1, dtype=torch.float64), 1) - torch.diag(torch.ones(n - 1, dtype=torch.float64), -1))
        if k == 0:
            G = torch.stack([L, I], dim=-1)[None]
        elif k == len(dims) - 1:
            G = torch.stack([I, L + I], dim=0)[..., None]
        else:
            G = torch.zeros((2, n, n, 2), dtype=torch.float64)
            G[0, :, :, 0], G[1, :, :, 0], G[1, :, :, 1] = I, L, I
        cores.append(G.to(dt).to(dev))
    return cores


def step_rows(args, dev):
    from tntorch_amd import _hipops, _hostops

    inner, A, I = 10, 2, 64
    for dt in (torch.float32, torch.float64):
        for R in (16, 32, 64):
            g = torch.Generator().manual_seed(R)
            G = laplace_cores([I] * 3, dt, dev)[1]
            eye = torch.eye(R, dtype=dt, device=dev)
            Phi = torch.stack([eye, eye], dim=1).contiguous()                   # [R, 2, R]: B = 2 I + 0.25 L on the mode
            Psi = Phi.clone()
            shape, n = (R, I, R), R * I * R
            v, r, Bp = (torch.randn(n, dtype=torch.float64, generator=g).to(dt).to(dev) for _ in range(3))
            p = r.clone()
            state = torch.zeros(8, dtype=torch.float64, device=dev)
            state[0] = torch.dot(r.double(), r.double())
            part = torch.zeros((2, _hipops.cg_parts(dt, n)), dtype=torch.float64, device=dev)
            part1 = torch.zeros((2, _hostops.cg_parts(dt, n)), dtype=torch.float64, device=dev)    # the mirror sums in one piece
            parts = {_hipops: part, _hostops: part1}

            def cg(ops, s):
                ops.cg_dot(p, Bp, parts[ops])
                ops.cg_update(s, p, Bp, v, r, parts[ops], state)
                ops.cg_direction(s, r, p, parts[ops], state)

            def step(ops, s):
                Bp.copy_(_hipops.local_matvec(Phi, G, Psi, p.view(shape)).reshape(-1))
                cg(ops, s)

            # step 0 runs untimed: the windows start at step 1 from a live state (rs in slot 1, part filled by both variants)
            step(_hostops, 0)
            Bp.copy_(_hipops.local_matvec(Phi, G, Psi, p.view(shape)).reshape(-1))
            _hipops.cg_dot(p, Bp, part)
            _hostops.cg_dot(p, Bp, part1)
            part[1, 0:1].copy_(state[1:2])       # what `direction` alone finishes: rs' = rs, beta = 1
            part1[1, 0:1].copy_(state[1:2])
            vs = [v, r, p, Bp, state, part, part1]
            keep = [t.clone() for t in vs]
            frozen = state.clone()
            frozen[2] = 2 * frozen[1]

            def restore():
                for t, k in zip(vs, keep):
                    t.copy_(k)

            def many(f):
                def run():
                    for s in range(1, inner + 1):
                        f(s)
                return run

            fns = {"cg": many(lambda s: cg(_hipops, s)), "cg_torch": many(lambda s: cg(_hostops, s)),
                   "step": many(lambda s: step(_hipops, s)), "step_torch": many(lambda s: step(_hostops, s)),
                   "dot": many(lambda s: _hipops.cg_dot(p, Bp, part)),
                   "update": many(lambda s: _hipops.cg_update(1, p, Bp, v, r, part, state)),
                   "update_frozen": many(lambda s: _hipops.cg_update(1, p, Bp, v, r, part, frozen)),
                   "direction": many(lambda s: _hipops.cg_direction(1, r, p, part, state))}
            ms, _ = alternate(fns, args.reps, before=restore)
            ms = {k: {q: t / inner for q, t in d.items()} for k, d in ms.items()}
            es = 4 if dt == torch.float32 else 8
            emit({"kind": "step", "dtype": str(dt), "R": R, "I": I, "A": A, "n": n, "reps": args.reps, "inner": inner,
                  "parts": _hipops.cg_parts(dt, n), "ms": ms,
                  "ratio_cg_torch_over_cg": ms["cg_torch"]["median_ms"] / ms["cg"]["median_ms"],
                  "ratio_step_torch_over_step": ms["step_torch"]["median_ms"] / ms["step"]["median_ms"],
                  "gbytes_per_s": {"dot": 2 * n * es / ms["dot"]["median_ms"] / 1e6, "update": 6 * n * es / ms["update"]["median_ms"] / 1e6,
                                   "direction": 3 * n * es / ms["direction"]["median_ms"] / 1e6,
                                   "cg": 11 * n * es / ms["cg"]["median_ms"] / 1e6},
                  "finite": bool(torch.isfinite(state).all() and torch.isfinite(v).all())})


class TorchCg:
    """The device ops with ``ttsolve._cg`` as the local solver: the baseline of the whole rows."""

    def __init__(self, ops):
        self.ops = ops

    def __getattr__(self, name):
        return getattr(self.ops, name)

    def cg_solve(self, Phi, Ak, Psi, f, x0, rel, iters, stat):
        from tntorch_amd.ttsolve import _cg

        return _cg(self.ops, Phi, Ak, Psi, f, x0, rel, iters, stat)


def whole_rows(args, dev):
    import tntorch_amd as tn
    from tntorch_amd import _hipops, ttamen

    real_ops_for = ttamen.ops_for
    baseline = TorchCg(_hipops)

    def with_ops(ops, fn):
        def f():
            ttamen.ops_for = lambda t, grad=False: ops
            try:
                return fn()
            finally:
                ttamen.ops_for = real_ops_for
        return f

    for dt in (torch.float32, torch.float64):
        for name, dims in (("64^8", [64] * 8), ("16^6", [16] * 6)):
            A = tn.TTMatrix(laplace_cores(dims, dt, dev), None, dims, dims)
            g = torch.Generator().manual_seed(len(dims))
            rk = [1] + [2] * (len(dims) - 1) + [1]
            b = tn.Tensor([torch.randn((rk[k], n, rk[k + 1]), dtype=torch.float64, generator=g).to(dt).to(dev) for k, n in enumerate(dims)])
            amen = lambda: tn.tt_amen_solve(A, b, return_info=True)  # noqa: E731
            x, info = amen()
            ranks = [int(q) for q in x.ranks_tt][1:-1]
            torch.manual_seed(len(dims) * 100)
            x0 = tn.rand(dims, ranks_tt=ranks)
            x0 = tn.Tensor([c.to(dt).to(dev) for c in x0.cores])
            fns = {"tt_amen_solve": amen, "cg_torch": with_ops(baseline, amen),
                   "tt_solve": lambda: tn.tt_solve(A, b, x0=x0, return_info=True)}
            ms, last = alternate(fns, args.whole_reps)
            emit({"kind": "whole", "operator": name, "dtype": str(dt), "ranks": ranks, "ranks_before_rounding": info["ranks"][-1],
                  "reps": args.whole_reps, "ms": ms,
                  "info": {k: {q: last[k][1][q] for q in ("sweeps", "converged", "residual")} for k in last},
                  "ratio_cg_torch_over_tt_amen_solve": ms["cg_torch"]["median_ms"] / ms["tt_amen_solve"]["median_ms"],
                  "ratio_tt_solve_over_tt_amen_solve": ms["tt_solve"]["median_ms"] / ms["tt_amen_solve"]["median_ms"]})


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["step", "whole"], default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--whole-reps", type=int, default=3)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("amen_bench needs a GPU")
    OUT = args.out
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    if args.only in (None, "step"):
        step_rows(args, dev)
    if args.only in (None, "whole"):
        whole_rows(args, dev)


if __name__ == "__main__":
    main()

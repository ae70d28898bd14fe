"""``tn.tt_eigsh`` and its kernels ``ttr_ritz_gram`` / ``ttr_ritz_update`` on one MI355X.  Reads nothing but this package.

    python tools/eigs_bench.py                      # every row
    python tools/eigs_bench.py --only step --reps 20
    python tools/eigs_bench.py --only whole
    python tools/eigs_bench.py --bounds             # no GPU: the worst cases recorded in tests/eigs_cases.py, from the host mirror

Step rows (``kind: step``): one Rayleigh-Ritz step of the local LOBPCG on vectors of n = R I S elements, R = S in {16, 32, 64},
I = 64, A = 2, fp32 and fp64, for a symmetric local operator with ``randn`` factors:
  ritz            ``_hipops.ritz_gram`` + ``_hipops.ritz_update`` (2 launches)
  ritz_torch      the host mirror's code (``_hostops.ritz_gram`` / ``ritz_update``, its two ``eigh`` included) on device tensors
  step            the matvec ``_hipops.local_matvec`` (2 launches) and ``ritz``
  step_torch      ``_hostops.local_matvec`` (einsum) and ``ritz_torch``
  gram, update    each kernel alone on a preallocated ``part`` (no allocation inside the window); ``update_frozen``: the update
                  with ``rel`` above the residual, which sums the partials and leaves before the pencil and the vectors
                  (update - update_frozen at small n: the serial 3 x 3 solve and the vector pass)
A timed window is ``inner`` consecutive steps between device events from the same restored vectors, the variants alternate
inside the repetition loop, and the figure is the median over --reps of window / inner.  ``gbytes_per_s``: 6 n elements read by
the Gram kernel, 6 n read and 5 n written by the update.

Whole rows (``kind: whole``): ``tn.tt_eigsh`` (which="SA", nswp=2, default tol and local_iters) of I + 0.25 sum_k L_k,
L = tridiag(-1, 2, -1), on [64]^8 and [16]^6 at ranks 16 and 32, fp32 and fp64 (median of --whole-reps, alternating):
  tt_eigsh    as a user calls it
  torch_ops   the same driver (tteigs.py) with every op from torch on the same GPU (the host mirror on device tensors)
and the split of one instrumented ``tt_eigsh`` (device events around every op call) into ``matvec``, ``qr_env`` (QR steps and
interface updates), ``ritz`` (the two kernels) and ``rest`` (the remaining wall time: allocation, copies, Python).
One JSON line per row, appended to profiles/eigs_bench_mi355x.jsonl.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "eigs_bench_mi355x.jsonl")


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


def step_rows(args, dev):
    from tntorch_amd import _hip, _hipops, _hostops

    inner, A, I = 10, 2, 64
    for dt in (torch.float32, torch.float64):
        for R in (16, 32, 64):
            g = torch.Generator().manual_seed(R)
            draw = lambda *s: (torch.randn(s, dtype=torch.float64, generator=g) / s[-1] ** 0.5).to(dt).to(dev)  # noqa: E731
            Phi, Psi, G = draw(R, A, R), draw(R, A, R), draw(A, I, I, A)
            Phi, Psi, G = Phi + Phi.permute(2, 1, 0), Psi + Psi.permute(2, 1, 0), G + G.permute(0, 2, 1, 3)   # a symmetric B
            shape, n = (R, I, R), R * I * R
            x = draw(*shape)
            state = torch.zeros(8, dtype=torch.float64, device=dev)
            sweep = torch.zeros(4, dtype=torch.float64, device=dev)
            vs = [torch.zeros(n, dtype=dt, device=dev) for _ in range(6)]      # X AX W AW P AP
            vs[0].copy_(x.reshape(-1))
            vs[1].copy_(_hipops.local_matvec(Phi, G, Psi, x).reshape(-1))
            _hipops.ritz_update(_hipops.RITZ_INIT, 0, 0, 0.0, _hipops.ritz_gram(_hipops.RITZ_INIT, vs[0], vs[1]), vs[0], vs[1], vs[2],
                                None, vs[4], vs[5], state, sweep)
            vs[3].copy_(_hipops.local_matvec(Phi, G, Psi, vs[2].reshape(shape)).reshape(-1))
            _hipops.ritz_update(_hipops.RITZ_STEP, 0, 1, 0.0, _hipops.ritz_gram(_hipops.RITZ_STEP, *vs), *vs, state, sweep)   # P != 0
            vs[3].copy_(_hipops.local_matvec(Phi, G, Psi, vs[2].reshape(shape)).reshape(-1))
            keep = [v.clone() for v in vs]
            part = _hipops.ritz_gram(_hipops.RITZ_STEP, *vs)

            def restore():
                for v, k in zip(vs, keep):
                    v.copy_(k)

            def ritz(ops, rel=0.0):
                ops.ritz_update(ops.RITZ_STEP, 0, 1, rel, ops.ritz_gram(ops.RITZ_STEP, *vs), *vs, state, sweep)

            def step(ops):
                vs[3].copy_(ops.local_matvec(Phi, G, Psi, vs[2].reshape(shape)).reshape(-1))
                ritz(ops)

            def many(f):
                def g():
                    for _ in range(inner):
                        f()            # the result is dropped at once: no window keeps a returned tensor alive
                return g

            fns = {"ritz": many(lambda: ritz(_hipops)), "ritz_torch": many(lambda: ritz(_hostops)),
                   "step": many(lambda: step(_hipops)), "step_torch": many(lambda: step(_hostops)),
                   "gram": many(lambda: _hip.ritz_gram(_hipops.RITZ_STEP, *vs, part=part)),
                   "update": many(lambda: _hipops.ritz_update(_hipops.RITZ_STEP, 0, 1, 0.0, part, *vs, state, sweep)),
                   "update_frozen": many(lambda: _hipops.ritz_update(_hipops.RITZ_STEP, 0, 1, 2.0, part, *vs, state, sweep))}
            ms, _ = alternate(fns, args.reps, before=restore)
            ms = {k: {q: v / inner for q, v in d.items()} for k, d in ms.items()}
            es = 4 if dt == torch.float32 else 8
            emit({"kind": "step", "dtype": str(dt), "R": R, "I": I, "A": A, "n": n, "reps": args.reps, "inner": inner,
                  "parts": _hipops.ritz_parts(dt, n), "ms": ms,
                  "ratio_ritz_torch_over_ritz": ms["ritz_torch"]["median_ms"] / ms["ritz"]["median_ms"],
                  "ratio_step_torch_over_step": ms["step_torch"]["median_ms"] / ms["step"]["median_ms"],
                  "gbytes_per_s": {"gram": 6 * n * es / ms["gram"]["median_ms"] / 1e6, "update": 11 * n * es / ms["update"]["median_ms"] / 1e6,
                                   "ritz": 17 * n * es / ms["ritz"]["median_ms"] / 1e6},
                  "update_minus_frozen_us": 1e3 * (ms["update"]["median_ms"] - ms["update_frozen"]["median_ms"]),
                  "finite": bool(torch.isfinite(state).all())})


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


class TimedOps:
    """The ops module with device events around every call, summed per share."""

    SHARES = {"local_matvec": "matvec", "left_orthogonalize": "qr_env", "right_orthogonalize": "qr_env", "env_update": "qr_env",
              "ritz_gram": "ritz", "ritz_update": "ritz"}

    def __init__(self, ops):
        self.ops, self.events = ops, []

    def __getattr__(self, name):
        fn = getattr(self.ops, name)
        share = self.SHARES.get(name)
        if share is None:
            return fn

        def wrapped(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **kw)
            e1.record()
            self.events.append((share, e0, e1))
            return out
        return wrapped

    def totals(self):
        torch.cuda.synchronize()
        out = {"matvec": 0.0, "qr_env": 0.0, "ritz": 0.0}
        for share, e0, e1 in self.events:
            out[share] += e0.elapsed_time(e1)
        return out


def whole_rows(args, dev):
    import tntorch_amd as tn
    from tntorch_amd import _hipops, _hostops, tteigs

    real_ops_for = tteigs.ops_for

    def with_ops(ops, fn):
        def f():
            tteigs.ops_for = (lambda t, grad=False: ops) if ops is not None else real_ops_for
            try:
                return fn()
            finally:
                tteigs.ops_for = real_ops_for
        return f

    for dt in (torch.float32, torch.float64):
        for name, dims in (("64^8", [64] * 8), ("16^6", [16] * 6)):
            for r in (16, 32):
                A = tn.TTMatrix(laplace_cores(dims, dt, dev), None, dims, dims)
                torch.manual_seed(len(dims) * 100 + r)
                x0 = tn.rand(dims, ranks_tt=r)
                x0 = tn.Tensor([c.to(dt).to(dev) for c in x0.cores])
                solve = lambda: tn.tt_eigsh(A, x0=x0, nswp=2, return_info=True)  # noqa: E731
                fns = {"tt_eigsh": solve, "torch_ops": with_ops(_hostops, solve)}
                ms, last = alternate(fns, args.whole_reps)
                timer = TimedOps(_hipops)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with_ops(timer, solve)()
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                shares = timer.totals()
                shares["rest"] = max(0.0, wall - sum(shares.values()))
                emit({"kind": "whole", "operator": name, "dtype": str(dt), "rank": r, "ranks": last["tt_eigsh"][1].ranks_tt.tolist(),
                      "nswp": 2, "reps": args.whole_reps, "ms": ms,
                      "value": {k: float(last[k][0]) for k in last}, "info": {k: last[k][2] for k in last},
                      "ratio_torch_ops_over_tt_eigsh": ms["torch_ops"]["median_ms"] / ms["tt_eigsh"]["median_ms"],
                      "instrumented_wall_ms": wall, "share_ms": shares,
                      "share_fraction": {k: v / wall for k, v in shares.items()}})


def bounds():
    """The worst value error and dense residual of the host mirror over the cases of tests/eigs_cases.py, seeds 0 .. 4."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import eigs_cases as ec
    import tntorch_amd as tn

    for dt in ec.DTYPES:
        worst_value = worst_residual = 0.0
        for name, ranks in ec.checked_cases():
            for which in ec.WHICH:
                for seed in range(5):
                    x0 = ec.start(name, dt, ranks, seed)
                    value, x, info = tn.tt_eigsh(ec.matrix(name, dt), x0=x0, which=which, tol=ec.TOL[dt], return_info=True)
                    worst_value = max(worst_value, ec.value_error(name, dt, which, value))
                    worst_residual = max(worst_residual, ec.dense_residual(name, dt, value, x))
        print(json.dumps({"kind": "bounds", "dtype": str(dt), "value_error": worst_value, "residual": worst_residual}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["step", "whole"], default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--whole-reps", type=int, default=3)
    ap.add_argument("--bounds", action="store_true")
    args = ap.parse_args()
    if args.bounds:
        return bounds()
    if not torch.cuda.is_available():
        sys.exit("eigs_bench needs a GPU")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if args.only in (None, "step"):
        step_rows(args, dev)
    if args.only in (None, "whole"):
        whole_rows(args, dev)


if __name__ == "__main__":
    main()

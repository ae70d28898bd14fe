"""``tn.tt_solve`` and its kernel ``ttr_env_half_apply`` on one MI355X.  Reads nothing but this package.

    python tools/solve_bench.py                     # every row
    python tools/solve_bench.py --only matvec --reps 20
    python tools/solve_bench.py --only whole

Matvec rows (``kind: matvec``): one application of the local operator, y = B_k v, for R = R' = S = S' in {16, 32, 64}, A = A' in
{2, 4, 8} and I = J in {8, 32, 64}, fp32 and fp64, operands ``randn``:
  fused      ``_hipops.local_matvec``: ttr_env_half_apply and one ttr_gemm on H as it lies (2 launches)
  unfused    the same H from the kernels the library had before (``_hipops.env_half_apply_unfused``: ttr_gemm, a permuted copy,
             ttr_ttm_step with a permuted copy of the core, a permuted copy), then the same ttr_gemm
  einsum     the three einsums in torch on the same GPU
Each variant is warmed up, the variants alternate inside the repetition loop, a timed window is ``inner`` calls back to back
between device events, and the figure is the median over --reps of window / inner.  ``ratio_*_over_fused`` >= 1: the fused
route is not slower.  The largest difference to the einsum relative to the largest entry is recorded.

Whole rows (``kind: whole``): ``tn.tt_solve`` of (I + 0.25 sum_k L_k) x = b, L = tridiag(-1, 2, -1), b a random rank-2 train, for
the shapes [64]^8 and [16]^6 and ranks 16 and 32, default ``tol``, ``nswp=4``, fp32 and fp64 (median of --whole-reps, alternating):
  tt_solve   as a user calls it
  torch_ops  the same driver (ttsolve.py) with every op -- matvec, environment updates, QR -- from torch on the same GPU
             (the host mirror's einsum / linalg.qr code run on device tensors)
and the split of one instrumented ``tt_solve`` (device events around every op call, which costs some overlap) into three shares:
``matvec`` (the local_matvec launches), ``qr_env`` (QR steps, environment and right-hand-side updates) and ``cg_torch`` (the
rest of the wall time: CG's vector and scalar ops, which torch runs).
One JSON line per row, appended to profiles/solve_bench_mi355x.jsonl.
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
OUT = os.path.join(ROOT, "profiles", "solve_bench_mi355x.jsonl")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def alternate(fns, reps):
    """Median ms of every variant, the variants taking turns inside each repetition; and the last result of each."""
    ts, last = {k: [] for k in fns}, {}
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in fns.items():
            ms, last[k] = timed(fn)
            ts[k].append(ms)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ts.items()}, last


def repeated(fn, inner):
    def f():
        for _ in range(inner):
            out = fn()
        return out
    return f


def emit(line):
    print(json.dumps(line), flush=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(line) + "\n")


def matvec_rows(args, dev):
    from tntorch_amd import _hipops

    def unfused(Phi, G, Psi, v):
        H = _hipops.env_half_apply_unfused(Phi, v, G)
        R, I, Ap, Sp = H.shape
        return _hipops.gemm2d(H.reshape(R * I, Ap * Sp), Psi.reshape(-1, Ap * Sp), transB=True).reshape(R, I, -1)

    def einsum(Phi, G, Psi, v):
        T = torch.einsum("rab,bjs->rajs", Phi, v)
        H = torch.einsum("rajs,aijc->rics", T, G)
        return torch.einsum("rics,tcs->rit", H, Psi)

    inner = 20
    for dt in (torch.float32, torch.float64):
        for R in (16, 32, 64):
            for A in (2, 4, 8):
                for I in (8, 32, 64):
                    g = torch.Generator().manual_seed(R * 1000 + A * 100 + I)
                    draw = lambda *s: (torch.randn(s, dtype=torch.float64, generator=g) / s[-1] ** 0.5).to(dt).to(dev)  # noqa: E731
                    Phi, Psi, G, v = draw(R, A, R), draw(R, A, R), draw(A, I, I, A), draw(R, I, R)
                    fns = {"fused": repeated(lambda: _hipops.local_matvec(Phi, G, Psi, v), inner),
                           "unfused": repeated(lambda: unfused(Phi, G, Psi, v), inner),
                           "einsum": repeated(lambda: einsum(Phi, G, Psi, v), inner)}
                    ms, last = alternate(fns, args.reps)
                    ms = {k: {q: x / inner for q, x in d.items()} for k, d in ms.items()}
                    top = float(last["einsum"].abs().max())
                    emit({"kind": "matvec", "dtype": str(dt), "R": R, "A": A, "I": I, "reps": args.reps, "inner": inner,
                          "flops_stage1": 2 * R * R * A * I * R, "flops_stage2": 2 * R * R * A * I * I * A, "ms": ms,
                          "ratio_unfused_over_fused": ms["unfused"]["median_ms"] / ms["fused"]["median_ms"],
                          "ratio_einsum_over_fused": ms["einsum"]["median_ms"] / ms["fused"]["median_ms"],
                          "largest_difference_over_largest_entry": {k: float((last[k] - last["einsum"]).abs().max()) / top
                                                                    for k in ("fused", "unfused")}})


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
              "gemm2d": "qr_env"}

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
        out = {"matvec": 0.0, "qr_env": 0.0}
        for share, e0, e1 in self.events:
            out[share] += e0.elapsed_time(e1)
        return out


def whole_rows(args, dev):
    import tntorch_amd as tn
    from tntorch_amd import _hipops, _hostops, ttsolve

    real_ops_for = ttsolve.ops_for

    def with_ops(ops, fn):
        def f():
            ttsolve.ops_for = (lambda t, grad=False: ops) if ops is not None else real_ops_for
            try:
                return fn()
            finally:
                ttsolve.ops_for = real_ops_for
        return f

    for dt in (torch.float32, torch.float64):
        for name, dims in (("64^8", [64] * 8), ("16^6", [16] * 6)):
            for r in (16, 32):
                N = len(dims)
                g = torch.Generator().manual_seed(N * 100 + r)
                A = tn.TTMatrix(laplace_cores(dims, dt, dev), None, dims, dims)
                rk = [1] + [2] * (N - 1) + [1]
                b = tn.Tensor([torch.randn((rk[k], n, rk[k + 1]), dtype=torch.float64, generator=g).to(dt).to(dev) for k, n in enumerate(dims)])
                x0 = tn.rand(dims, ranks_tt=r)
                x0 = tn.Tensor([c.to(dt).to(dev) for c in x0.cores])
                solve = lambda: tn.tt_solve(A, b, x0=x0, nswp=4, return_info=True)  # noqa: E731
                fns = {"tt_solve": solve, "torch_ops": with_ops(_hostops, solve)}
                ms, last = alternate(fns, args.whole_reps)
                torch.cuda.synchronize()
                timer = TimedOps(_hipops)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with_ops(timer, solve)()
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                shares = timer.totals()
                shares["cg_torch"] = max(0.0, wall - shares["matvec"] - shares["qr_env"])
                emit({"kind": "whole", "operator": name, "dtype": str(dt), "rank": r, "ranks": last["tt_solve"][0].ranks_tt.tolist(),
                      "nswp": 4, "reps": args.whole_reps, "ms": ms,
                      "info": {k: {q: v for q, v in last[k][1].items()} for k in last},
                      "ratio_torch_ops_over_tt_solve": ms["torch_ops"]["median_ms"] / ms["tt_solve"]["median_ms"],
                      "instrumented_wall_ms": wall, "share_ms": shares,
                      "share_fraction": {k: v / wall for k, v in shares.items()}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["matvec", "whole"], default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--whole-reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("solve_bench needs a GPU")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if args.only in (None, "matvec"):
        matvec_rows(args, dev)
    if args.only in (None, "whole"):
        whole_rows(args, dev)


if __name__ == "__main__":
    main()

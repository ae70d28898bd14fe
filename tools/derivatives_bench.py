"""Differential operators on a tensor train on one MI355X: the structured paths of tntorch_amd/derivatives.py next to the
reference's algorithms written with this package's own ``partial``, ``+``, ``*`` and ``dot``.

    python tools/derivatives_bench.py                     # 8 modes of 64, rank 32, fp32
    python tools/derivatives_bench.py --modes 6 --rank 16 --reps 5

Timed (ms per call, device events around work that ends in a synchronise; every variant is warmed up once, the variants of a
pair alternate inside the repetition loop, the figure is the median of --reps):
  laplacian    (a) ``tn.laplacian(t)`` (ranks 2 r) followed by ``round_tt(eps)``;
               (b) the sum of the N trains ``partial(t, n, order=2)`` (ranks N r) followed by the same rounding;
               each also without its rounding, and the relative distance between the two rounded results
  sensitivity  (c) ``tn.active_subspace(t, bounds)`` against the N (N + 1) / 2 calls ``tn.dot(g_i * pdf, g_j)`` on the N gradient
               trains (the gradient and the weight train built inside the timed call, as the reference does), and the largest
               difference between the two matrices relative to the largest entry
The train has ``rand`` cores scaled by 2 / rank.  One JSON line per run, appended to profiles/derivatives_bench_mi355x.jsonl.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "derivatives_bench_mi355x.jsonl")


def train(N, I, r, dtype, device, seed=0):
    import tntorch_amd as tn

    g = torch.Generator().manual_seed(seed)
    rs = [1] + [r] * (N - 1) + [1]
    return tn.Tensor([(torch.rand(rs[n], I, rs[n + 1], generator=g, dtype=torch.float64) * (2.0 / r)).to(dtype).to(device)
                      for n in range(N)])


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
    for k, fn in fns.items():   # warm-up: code objects, allocator
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in fns.items():
            ms, last[k] = timed(fn)
            ts[k].append(ms)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ts.items()}, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", type=int, default=8)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f32")
    ap.add_argument("--eps", type=float, default=1e-6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["laplacian", "sensitivity"], default=None)
    a = ap.parse_args()
    import tntorch_amd as tn
    from tntorch_amd import derivatives

    if not torch.cuda.is_available():
        sys.exit("derivatives_bench needs a GPU")
    dtype = torch.float32 if a.dtype == "f32" else torch.float64
    N = a.modes
    cfg = {"modes": N, "size": a.size, "rank": a.rank, "dtype": a.dtype, "eps": a.eps, "reps": a.reps}
    t = train(N, a.size, a.rank, dtype, torch.device("cuda:0"))
    bounds = [[0.0, 1.0 + 0.25 * n] for n in range(N)]
    lines = []

    if a.only in (None, "laplacian"):
        def summed():
            s = tn.partial(t, 0, order=2, bounds=bounds[0])
            for n in range(1, N):
                s = s + tn.partial(t, n, order=2, bounds=bounds[n])
            return s

        def rounded(build):
            def f():
                x = build()
                x.round_tt(eps=a.eps)
                return x
            return f

        structured = lambda: tn.laplacian(t, bounds=bounds)  # noqa: E731
        ms, last = alternate({"structured_build": structured, "summed_build": summed,
                              "structured_build_round": rounded(structured), "summed_build_round": rounded(summed)}, a.reps)
        sa, sb = last["structured_build_round"], last["summed_build_round"]
        lines.append({"config": cfg, "what": "laplacian", "ms": ms,
                      "ranks_before": {"structured": last["structured_build"].ranks_tt.tolist(), "summed": last["summed_build"].ranks_tt.tolist()},
                      "ranks_after": {"structured": sa.ranks_tt.tolist(), "summed": sb.ranks_tt.tolist()},
                      "relative_distance_of_rounded_results": float(tn.dist(sa, sb) / tn.norm(sb))})

    if a.only in (None, "sensitivity"):
        def reference_way():
            c0 = t.cores[0]
            w = []
            for I in t.shape:
                m = torch.full((I - 1,), 1.0 / (I - 1), dtype=c0.dtype, device=c0.device)
                w.append(torch.cat([m, m.new_zeros(1)])[None, :, None])
            pdf = tn.Tensor(w)
            grad = tn.gradient(t, bounds=bounds)
            e = {}
            for i in range(N):
                first = grad[i] * pdf
                for j in range(i, N):
                    e[(i, j)] = tn.dot(first, grad[j])
            return torch.stack([e[(min(i, j), max(i, j))] for i in range(N) for j in range(N)]).reshape(N, N)

        ms, last = alternate({"environments_matrix": lambda: derivatives._as_matrix(t, bounds, None),
                              "environments_with_eigh": lambda: tn.active_subspace(t, bounds),
                              "gradient_trains_and_dots_matrix": reference_way}, a.reps)
        Ma, Mb = last["environments_matrix"].double(), last["gradient_trains_and_dots_matrix"].double()
        lines.append({"config": cfg, "what": "active_subspace", "ms": ms,
                      "largest_difference_of_M_over_largest_entry": float((Ma - Mb).abs().max() / Mb.abs().max()),
                      "eigenvalues": last["environments_with_eigh"][0].tolist()})

    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        for line in lines:
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

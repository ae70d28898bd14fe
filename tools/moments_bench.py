"""Moments of a tensor train (tn.raw_moment) on one MI355X: ms per call on the device next to the CPU mirror.

    python tools/moments_bench.py                 # 8 modes of 64, rank 16, fp32: raw_moment(t, 3) and (t, 4), "eig" and "exact"
    python tools/moments_bench.py --no-cpu --orders 3 --algorithms eig

The train has ``rand`` cores scaled by 2 / rank (positive entries: the moments are well conditioned).  Device time
is the best of --reps calls between HIP events after one warm-up call.  The CPU mirror is the same algorithm restated in torch
on CPU tensors (tntorch_amd's host path: the reference itself only runs in fp32 on the CPU and returns through ``.item()``);
one call, wall clock.  For the "eig" runs two breakdowns of one further call are recorded:
  stages   HIP events around the three stages of the approximate path as the Python layer enqueues them: the roundings
           (``round_tt``), the contraction between them (``core_matvec`` = ttr_core_matvec) and the diagonal cores (``diag_cores``,
           torch indexing); "other" is what remains of the call (the final GEMM chain, gaps)
  kinds    the library's per-kind device times (ttr_prof_enable(1)); ttr_core_matvec / ttr_hsum_step are counted under "misc",
           together with the small streaming kernels of the sweeps
One JSON line per run.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def train(N, I, r, dtype, device, seed=0):
    import tntorch_amd as tn

    g = torch.Generator().manual_seed(seed)
    rs = [1] + [r] * (N - 1) + [1]
    return tn.Tensor([(torch.rand(rs[n], I, rs[n + 1], generator=g, dtype=torch.float64) * (2.0 / r)).to(dtype).to(device)
                      for n in range(N)])


def time_device(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        v = fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return min(ts), float(v)


def stage_times(fn):
    """One call with HIP events around every round_tt / core_matvec / diag_cores the Python layer enqueues."""
    from tntorch_amd import _hipops

    spans = {"round_tt": [], "core_matvec": [], "diag_cores": []}
    saved = {k: getattr(_hipops, k) for k in spans}
    ranks = []

    def wrap(name):
        def f(*args, **kw):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = saved[name](*args, **kw)
            b.record()
            spans[name].append((a, b))
            if name == "round_tt":
                ranks.append([[int(c.shape[1]) for c in args[0]][1:], [int(c.shape[1]) for c in out][1:]])
            return out
        return f

    for k in spans:
        setattr(_hipops, k, wrap(k))
    try:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
    finally:
        for k, f in saved.items():
            setattr(_hipops, k, f)
    total = a.elapsed_time(b)
    out = {k: sum(x.elapsed_time(y) for x, y in v) for k, v in spans.items()}
    out["other"] = total - sum(out.values())
    out["total"] = total
    out["bonds_in_out_per_rounding"] = ranks
    return out


def kind_times(fn):
    from tntorch_amd import _hip

    _hip.prof_enable(1)
    try:
        _hip.prof_collect()
        fn()
        torch.cuda.synchronize()
        return {k: v for k, v in _hip.prof_collect().items() if v["launches"]}
    finally:
        _hip.prof_enable(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", type=int, default=8)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--orders", type=int, nargs="+", default=[3, 4])
    ap.add_argument("--algorithms", nargs="+", default=["exact", "eig"], choices=["exact", "eig", "svd"])
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f32")
    ap.add_argument("--eps", type=float, default=1e-6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--cpu-only", action="store_true")
    a = ap.parse_args()
    import tntorch_amd as tn

    dtype = torch.float32 if a.dtype == "f32" else torch.float64
    cfg = {"modes": a.modes, "size": a.size, "rank": a.rank, "dtype": a.dtype, "eps": a.eps}
    if not a.cpu_only:
        if not torch.cuda.is_available():
            sys.exit("moments_bench needs a GPU (or --cpu-only)")
        t = train(a.modes, a.size, a.rank, dtype, torch.device("cuda:0"))
    if not a.no_cpu:
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        tc = train(a.modes, a.size, a.rank, dtype, torch.device("cpu"))
    for alg in a.algorithms:   # (the cheap runs first: every finished run has its line out)
        for k in a.orders:
            out = {"config": cfg, "order": k, "algorithm": alg}
            if not a.cpu_only:
                fn = lambda: tn.raw_moment(t, k, eps=a.eps, algorithm=alg)  # noqa: E731
                fn()  # warm-up: code objects, allocator
                torch.cuda.synchronize()
                ms, v = time_device(fn, a.reps)
                out["device"] = {"ms": ms, "value": v}
                if alg != "exact":
                    out["device"]["stages_ms"] = stage_times(fn)
                out["device"]["kinds"] = kind_times(fn)
            if not a.no_cpu:
                t0 = time.perf_counter()
                v = float(tn.raw_moment(tc, k, eps=a.eps, algorithm=alg))
                out["cpu_mirror"] = {"ms": (time.perf_counter() - t0) * 1e3, "value": v, "threads": torch.get_num_threads()}
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

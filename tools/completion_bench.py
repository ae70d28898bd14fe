"""TT completion (tn.als_completion) on one MI355X: ms per ALS sweep on the device (fp32 and fp64) next to the CPU mirror.

    python tools/completion_bench.py                       # N = 6 modes of 64, rank 8 (K = 64), P = 2^20, both dtypes
    python tools/completion_bench.py --profile --dtype f64 # one warm-up and one timed call only, for a separate
        rocprofv3 --kernel-trace --stats -d OUT -- python tools/completion_bench.py --profile ...

Device time comes from HIP events around whole calls; a sweep is the difference between a call with 1 + k sweeps and one with 1
sweep, divided by k (so the per-call set-up -- slice counts, sort, plans, initial orthogonalisation -- drops out).  The CPU mirror
runs the same train at --cpu-p samples (it cannot finish 2^20 in reasonable time); its per-sweep time is reported as measured,
not scaled.  One JSON line per run.

Model of one core step (ranks r0, r1, K = r0 r1, P samples), the flop / byte model DESIGN.md section 13 uses:
  ttr_als_normal  P K^2 FMAs if the whole K x K Gram were formed (2 P K^2 flops; the kernel forms the lower-triangle tiles,
                  (nT + 1) / (2 nT) of it, nT = ceil(K / 16)); reads P (r0 + r1 + 3) words (L, R, w, y) + 8 P bytes of permutation
  ttr_spd_solve   I K^3 / 3 FMAs, reads tasks x K^2 words of partial Grams
so the normal equations are compute-bound for K >~ 16: at K = 64 and fp64 it is 2 K^2 / ((r0 + r1 + 4) 8) ~ 43 flop/byte.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = {"f32": 157.3, "f64": 78.6}  # MI355X matrix-core peaks (AMD spec; fp32 inputs exact, no xf32)


def step_model(P, r0, r1, I, es):
    K = r0 * r1
    return {"flops_normal": 2.0 * P * K * K, "bytes_normal": P * ((r0 + r1 + 3) * es + 8), "flops_solve": 2.0 * I * K ** 3 / 3}


def sweep_model(P, N, I, r, es):
    """Sum over the 2 (N - 1) core steps of one sweep (left-to-right mu = 0 .. N-2, right-to-left mu = N-1 .. 1)."""
    ranks = [1] + [r] * (N - 1) + [1]
    mus = list(range(N - 1)) + list(range(N - 1, 0, -1))
    tot = {"flops_normal": 0.0, "bytes_normal": 0.0, "flops_solve": 0.0}
    for mu in mus:
        for k, v in step_model(P, ranks[mu], ranks[mu + 1], I, es).items():
            tot[k] += v
    return tot


def problem(N, I, r, P, device, dtype, seed=0):
    import tntorch_amd as tn

    g = torch.Generator().manual_seed(seed)
    rs = [1] + [r] * (N - 1) + [1]
    target = tn.Tensor([torch.randn(rs[n], I, rs[n + 1], generator=g, dtype=torch.float64) for n in range(N)])
    X = torch.randint(0, I, (P, N), generator=g)
    X[:I] = torch.arange(I)[:, None]  # every slice covered
    y = target.to(device)[X.to(device)].torch() if device.type != "cpu" else target[X].torch()
    return X.to(device), y.to(dtype), [torch.rand(rs[n], I, rs[n + 1], generator=g, dtype=torch.float64) for n in range(N)]


def run(X, y, init, niter, device, dtype):
    import tntorch_amd as tn

    x0 = tn.Tensor([c.to(device, dtype) for c in init])
    return tn.als_completion(X, y, ranks_tt=None, x0=x0, niter=niter, verbose=False)


def time_device(X, y, init, niter, dtype, reps):
    dev = X.device
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        run(X, y, init, niter, dev, dtype)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", type=int, default=6)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--rank", type=int, default=8)
    ap.add_argument("--p", type=int, default=1 << 20)
    ap.add_argument("--cpu-p", type=int, default=1 << 14)
    ap.add_argument("--sweeps", type=int, default=3, help="k: timed calls run 1 and 1 + k sweeps")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dtype", choices=["f32", "f64", "both"], default="both")
    ap.add_argument("--profile", action="store_true", help="one warm-up call and one 2-sweep call, nothing else")
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("completion_bench needs a GPU")
    dev = torch.device("cuda:0")
    N, I, r = a.modes, a.size, a.rank
    out = {"config": {"modes": N, "size": I, "rank": r, "K": r * r, "P": a.p, "sweeps_timed": a.sweeps}}
    for name in (["f32", "f64"] if a.dtype == "both" else [a.dtype]):
        dtype = torch.float32 if name == "f32" else torch.float64
        X, y, init = problem(N, I, r, a.p, dev, dtype)
        run(X, y, init, 1, dev, dtype)  # warm-up: code objects, allocator
        torch.cuda.synchronize()
        if a.profile:
            run(X, y, init, 2, dev, dtype)
            torch.cuda.synchronize()
            out[name] = {"profile_run": True}
            continue
        t1 = time_device(X, y, init, 1, dtype, a.reps)
        tk = time_device(X, y, init, 1 + a.sweeps, dtype, a.reps)
        ms = (tk - t1) / a.sweeps
        m = sweep_model(a.p, N, I, r, 4 if name == "f32" else 8)
        t = run(X, y, init, 1 + a.sweeps, dev, dtype)
        tc = tuple(c for c in t.cores)
        err = float(((t[X].torch() - y).double().norm() / y.double().norm()))
        out[name] = {"ms_per_sweep": ms, "ms_call_1_sweep": t1, "setup_plus_first_sweep_ms": t1,
                     "model_gflop_per_sweep": (m["flops_normal"] + m["flops_solve"]) / 1e9,
                     "model_tflops_end_to_end": (m["flops_normal"] + m["flops_solve"]) / (ms * 1e-3) / 1e12,
                     "share_of_matrix_peak_end_to_end": (m["flops_normal"] + m["flops_solve"]) / (ms * 1e-3) / 1e12 / PEAK_TFLOPS[name],
                     "train_rel_err": err, "ranks": [int(c.shape[0]) for c in tc] + [1]}
        del X, y
        torch.cuda.empty_cache()
    if not a.profile and not a.no_cpu:
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        X, y, init = problem(N, I, r, a.cpu_p, torch.device("cpu"), torch.float64)
        ts = []
        for niter in (1, 2):
            t0 = time.perf_counter()
            run(X, y, init, niter, torch.device("cpu"), torch.float64)
            ts.append(time.perf_counter() - t0)
        out["cpu_mirror_f64"] = {"P": a.cpu_p, "ms_per_sweep": (ts[1] - ts[0]) * 1e3}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

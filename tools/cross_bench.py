"""Time TT-cross on one GPU: ttr_maxvol alone (device vs the host mirror) and a full device cross.

    python tools/cross_bench.py [--reps 5]

Prints one JSON line per measurement.  maxvol: 2048 x 32 and 6400 x 100 random matrices, fp32 / fp64, default tol and max_iters;
``swaps`` is the number of row swaps the kernel made, ``launch_us`` the device time per launch (LU steps + swap launches + the
two solves), ``model_us`` what the C traffic of those launches costs at 5 TB/s (each LU / swap launch reads and writes the
N x r matrix once).  cross: 10 modes x 64 points, ranks_tt=32, 4 sweeps, fp32, f = 1 / (1 + sum c_k x_k).
Run it under ``rocprofv3 --kernel-trace --stats`` for the per-kernel breakdown.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tntorch_amd as tn  # noqa: E402
from tntorch_amd import _hip  # noqa: E402


def time_dev(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def time_host(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["maxvol", "cross"], default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    if a.only in (None, "maxvol"):
        for N, r in [(2048, 32), (6400, 100)]:
            for dt in (torch.float32, torch.float64):
                A = torch.randn(N, r, generator=torch.Generator().manual_seed(N), dtype=torch.float64).to(dt)
                Ad = A.to(dev)
                status = torch.zeros(1, 2, dtype=torch.int32, device=dev)
                ms = time_dev(lambda: _hip.maxvol(Ad[None], 1.05, 100, status=status), a.reps)
                swaps = int(status[0, 1])
                host = time_host(lambda: tn.maxvol(A), max(1, a.reps // 2))
                launches = (r + 1) + 101 + 4
                bytes_per = 2 * N * r * A.element_size()
                print(json.dumps({"bench": "maxvol", "N": N, "r": r, "dtype": str(dt).split(".")[-1], "device_ms": round(ms, 3),
                                  "host_ms": round(host, 3), "swaps": swaps, "launches": launches,
                                  "launch_us": round(ms * 1e3 / launches, 2),
                                  "model_us": round((r + 1 + swaps + 1) * bytes_per / 5e12 * 1e6, 2)}), flush=True)
    if a.only in (None, "cross"):
        domain = [torch.linspace(0, 1, 64, device=dev) for _ in range(10)]
        f = lambda *xs: 1 / (1 + sum((0.5 + 0.1 * k) * x for k, x in enumerate(xs)))

        def run():
            np.random.seed(0)
            torch.manual_seed(0)
            return tn.cross(f, domain=domain, ranks_tt=32, max_iter=4, eps=1e-30, verbose=False, return_info=True,
                            suppress_warnings=True)

        ms = time_dev(run, max(1, a.reps // 2))
        _, info = run()
        print(json.dumps({"bench": "cross", "modes": 10, "I": 64, "ranks_tt": 32, "sweeps": len(info["val_epss"]),
                          "ms": round(ms, 2), "ms_per_sweep": round(ms / len(info["val_epss"]), 2),
                          "val_eps": float(info["val_eps"]), "nsamples": info["nsamples"]}), flush=True)


if __name__ == "__main__":
    main()

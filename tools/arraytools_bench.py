"""``ttr_mode_scan`` and ``ttr_mode_reduce`` on one MI355X next to torch on the same device tensors, and next to the route a
vector ``ttm`` had before (``mode_mul`` with a ``[1, I]`` factor: one M = 1 GEMM per rank slice).

    python tools/arraytools_bench.py
    python tools/arraytools_bench.py --reps 9 --inner 50

Per shape (R, I, C) of (64, 64, 64), (64, 1024, 64), (1, 4096, 64), (64, 4096, 1) and dtype (fp32, fp64), median ms per launch:
  scan     ``_hip.mode_scan(X)``                      against ``torch.cumsum(X, 1)``
  reduce   ``_hip.mode_reduce(X, w)``                 against ``(X * w[None, :, None]).sum(1)`` and ``_hipops.mode_mul(X[None], w[None, None])``
Every variant writes into a fresh result, is warmed up once, and is timed as ``--inner`` back-to-back launches between two
device events (a single launch of these sizes is shorter than the clock's noise); the variants of a group alternate inside the
repetition loop, the figure is the median of ``--reps`` divided by ``--inner``.  The byte models are those of DESIGN section 19
(scan: 2 R I C sizeof, reduce: R I C sizeof); ``fraction_of_6.3TBps`` is bytes / time over the 6.3 TB/s a streaming kernel
reaches on this part.  A core of these sizes (1 to 32 MiB) fits the 256 MiB Infinity Cache and the launches repeat on the same
buffers, so these are times with the input cache-resident, not HBM rates.  The largest difference between the results of the
variants is recorded.  One JSON line per shape and dtype, appended to profiles/arraytools_bench_mi355x.jsonl.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "arraytools_bench_mi355x.jsonl")
SHAPES = [(64, 64, 64), (64, 1024, 64), (1, 4096, 64), (64, 4096, 1)]
STREAM_BYTES_PER_S = 6.3e12


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(inner):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner, out


def alternate(fns, reps, inner):
    """Median ms per launch of every variant, the variants taking turns inside each repetition; and the last result of each."""
    ts, last = {k: [] for k in fns}, {}
    for fn in fns.values():   # warm-up: code objects, allocator
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in fns.items():
            ms, last[k] = timed(fn, inner)
            ts[k].append(ms)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ts.items()}, last


def with_model(ms, nbytes):
    for v in ms.values():
        v["GBps_of_byte_model"] = nbytes / (v["median_ms"] * 1e-3) / 1e9
        v["fraction_of_6.3TBps"] = nbytes / (v["median_ms"] * 1e-3) / STREAM_BYTES_PER_S
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("arraytools_bench needs a GPU")
    from tntorch_amd import _hip, _hipops

    lines = []
    for dtype, name in ((torch.float32, "f32"), (torch.float64, "f64")):
        for shape in SHAPES:
            R, I, C = shape
            g = torch.Generator().manual_seed(0)
            X = torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype).cuda()
            w = torch.randn(I, generator=g, dtype=torch.float64).to(dtype).cuda()
            size = X.element_size()
            scan_ms, scan_out = alternate({"ttr_mode_scan": lambda: _hip.mode_scan(X), "torch_cumsum": lambda: torch.cumsum(X, 1)}, a.reps, a.inner)
            red_ms, red_out = alternate({"ttr_mode_reduce": lambda: _hip.mode_reduce(X, w),
                                         "torch_weighted_sum": lambda: (X * w[None, :, None]).sum(1),
                                         "mode_mul_row_factor": lambda: _hipops.mode_mul(X[None], w[None, None])}, a.reps, a.inner)
            line = {"config": {"shape": list(shape), "dtype": name, "reps": a.reps, "inner": a.inner},
                    "scan": {"byte_model": 2 * R * I * C * size, "ms": with_model(scan_ms, 2 * R * I * C * size),
                             "largest_difference": float((scan_out["ttr_mode_scan"] - scan_out["torch_cumsum"]).abs().max())},
                    "reduce": {"byte_model": R * I * C * size, "ms": with_model(red_ms, R * I * C * size),
                               "largest_difference_to_torch": float((red_out["ttr_mode_reduce"] - red_out["torch_weighted_sum"]).abs().max()),
                               "largest_difference_to_mode_mul": float((red_out["ttr_mode_reduce"] - red_out["mode_mul_row_factor"][0, :, 0, :]).abs().max())}}
            lines.append(line)
            print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

"""``tn.accepted_inputs`` on one MI355X: the level steps on ``ttr_accept_count`` / ``ttr_accept_expand`` next to the same level steps
written with torch ops on the device, and next to the CPU mirror.  Reads nothing but this package.

    python tools/accepted_bench.py                    # N = 16, 20, 24
    python tools/accepted_bench.py --only 20 --reps 10

Cases: ``weight_mask(N, N // 2)`` in fp32 for N = 16, 20 and 24: C(N, N / 2) = 12870, 184756 and 2704156 strings.
Per case (ms, device events around work that ends in a synchronise; every variant warmed up once, the variants alternate inside
the repetition loop, the figure is the median of --reps):
  kernels        tn.accepted_inputs(t) on the device as a user calls it (backward pass, N level steps, N + 2 host reads)
  torch_levels   the same loop with ``_hostops``' level steps (matmul, searchsorted, index) on DEVICE tensors: what torch offers
                 without the kernels (its consistency checks read the host once more per mode)
  cpu_mirror     tn.accepted_inputs on a CPU copy (host clock, one repetition after a warm-up)
  ratio_torch_over_kernels = torch_levels / kernels (>= 1: the kernels are not slower)
and ``equal``: the three results are the same matrix.  ``rows_per_s`` is S over the kernels' time, ``out_bytes`` the 8 S N bytes of
the result.  One JSON line per case, appended to profiles/accepted_bench_mi355x.jsonl.
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
OUT = os.path.join(ROOT, "profiles", "accepted_bench_mi355x.jsonl")


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
    for fn in fns.values():   # warm-up: code objects, allocator
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in fns.items():
            ms, last[k] = timed(fn)
            ts[k].append(ms)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ts.items()}, last


def torch_levels(t):
    """automata.accepted_inputs with the host mirror's level steps running on the device tensors."""
    from tntorch_amd import _hostops as ops

    cores = [c.contiguous() for c in t.cores]
    dev, N = cores[0].device, len(cores)
    fibers, right0 = ops.accept_fibers(cores)
    S = int(torch.round(right0.sum()).item())
    Xs = torch.empty((S, N), dtype=torch.int64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    L = torch.ones((1, cores[0].shape[0]), dtype=torch.float64, device=dev)
    off = torch.zeros(1, dtype=torch.int64, device=dev)
    cnt = torch.full((1,), S, dtype=torch.int64, device=dev)
    for mu in range(N):
        C = ops.accept_count(L, fibers[mu])
        childoff = off[:, None] + (torch.cumsum(C, dim=1) - C)
        productive = C.reshape(-1) > 0
        K = int(productive.sum().item())
        idx = torch.nonzero_static(productive, size=K).reshape(-1)
        L, off, cnt = ops.accept_expand(L, cores[mu], C, childoff, cnt, idx, Xs, mu, flag, mu == N - 1)
    assert int(flag.item()) == 0
    return Xs


def run_case(N, reps):
    import tntorch_amd as tn

    t = tn.weight_mask(N, N // 2, device="cuda")
    stats, last = alternate({"kernels": lambda: tn.accepted_inputs(t), "torch_levels": lambda: torch_levels(t)}, reps)
    tc = tn.weight_mask(N, N // 2)
    tn.accepted_inputs(tn.weight_mask(8, 4))
    t0 = time.perf_counter()
    ref = tn.accepted_inputs(tc)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    S = int(ref.shape[0])
    rec = {"case": "weight_mask({}, {})".format(N, N // 2), "N": N, "S": S, "dtype": "float32", "reps": reps,
           "kernels": stats["kernels"], "torch_levels": stats["torch_levels"], "cpu_mirror_ms": cpu_ms,
           "ratio_torch_over_kernels": stats["torch_levels"]["median_ms"] / stats["kernels"]["median_ms"],
           "rows_per_s": S / (stats["kernels"]["median_ms"] * 1e-3), "out_bytes": 8 * S * N,
           "equal": bool(torch.equal(last["kernels"].cpu(), ref) and torch.equal(last["torch_levels"].cpu(), ref)),
           "device": torch.cuda.get_device_name(0)}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", type=int, default=None, help="one N of 16, 20, 24")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("accepted_bench.py measures on an MI355X: no GPU is visible")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for N in (16, 20, 24):
        if args.only is not None and N != args.only:
            continue
        rec = run_case(N, args.reps)
        print(json.dumps(rec))
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

"""``ttr_pce_design`` and ``ttr_pce_predict`` on one MI355X next to the reference's formulation written with torch ops on the
same device tensors (the basis values of all points ``[P, N, S]``, a gather of the ``P x C x N`` factors, ``prod`` over the modes;
predict: that matrix times ``coef``), and next to the CPU mirror (``_hostops``, CPU tensors, host clock).

    python tools/pce_bench.py
    python tools/pce_bench.py --reps 7 --inner 10

Per shape (P, N, S, C) and dtype (fp32, fp64), median ms per call.  The device variants write into fresh results, are warmed up
once, and are timed as ``--inner`` back-to-back calls between two device events, taking turns inside the repetition loop; the
figure is the median of ``--reps`` divided by ``--inner``.  The CPU mirror is timed once per repetition with the host clock
(at most ``--cpu-reps`` times).  Models kept with the figures: design writes ``P C sizeof`` bytes (its least traffic, against
6.3 TB/s) and performs ``P C N`` fp64 multiplies on ``P C N`` LDS reads of 8 bytes; predict performs the same and ``P C`` FMAs
and writes ``P sizeof``.  The largest difference between the variants' results is recorded, relative to the largest entry.
One JSON line per shape and dtype, appended to profiles/pce_bench_mi355x.jsonl.
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
OUT = os.path.join(ROOT, "profiles", "pce_bench_mi355x.jsonl")
SHAPES = [(100000, 3, 4, 19), (100000, 5, 5, 100), (1000000, 5, 5, 100), (200000, 8, 4, 300)]   # (P, N, S, C)
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
    """Median ms per call of every variant, the variants taking turns inside each repetition; and the last result of each."""
    ts, last = {k: [] for k in fns}, {}
    for fn in fns.values():   # warm-up: code objects, allocator
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in fns.items():
            ms, last[k] = timed(fn, inner)
            ts[k].append(ms)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ts.items()}, last


def host_timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}, out


def torch_design(Z, Psi, coords):
    """The gather-and-prod formulation with torch ops: all basis values, the P x C x N factors, their product."""
    N, S = Psi.shape[0], Psi.shape[1]
    ks = torch.arange(S, device=Z.device)
    B = torch.stack([(Z[:, n, None] ** ks) @ Psi[n] for n in range(N)], dim=1)           # [P, N, S]
    modes = torch.arange(N, device=Z.device).expand(coords.shape[0], N)
    return B[:, modes.reshape(-1), coords.reshape(-1)].reshape(Z.shape[0], coords.shape[0], N).prod(dim=2)


def largest_difference(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--cpu-reps", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pce_bench needs a GPU")
    from tntorch_amd import _hip, _hostops

    lines = []
    for dtype, name in ((torch.float32, "f32"), (torch.float64, "f64")):
        for P, N, S, C in SHAPES:
            g = torch.Generator().manual_seed(0)
            Z = torch.randn(P, N, generator=g, dtype=torch.float64).to(dtype)
            Psi = (torch.triu(torch.randn(N, S, S, generator=g, dtype=torch.float64)) * 0.3 + torch.eye(S, dtype=torch.float64)).to(dtype)
            coords = torch.randint(0, S, (C, N), generator=g)
            coef = torch.randn(C, generator=g, dtype=torch.float64).to(dtype)
            Zd, Psid, cd, cfd = Z.cuda(), Psi.cuda(), coords.cuda(), coef.cuda()
            size = Z.element_size()
            des_ms, des_out = alternate({"ttr_pce_design": lambda: _hip.pce_design(Zd, Psid, cd)[0],
                                         "torch_gather_prod": lambda: torch_design(Zd, Psid, cd)}, a.reps, a.inner)
            pre_ms, pre_out = alternate({"ttr_pce_predict": lambda: _hip.pce_predict(Zd, Psid, cd, cfd)[0],
                                         "torch_gather_prod_matmul": lambda: torch_design(Zd, Psid, cd) @ cfd}, a.reps, a.inner)
            cpu_reps = min(a.cpu_reps, a.reps)
            des_ms["cpu_mirror"], cpu_M = host_timed(lambda: _hostops.pce_design(Z, Psi, coords), cpu_reps)
            pre_ms["cpu_mirror"], cpu_y = host_timed(lambda: _hostops.pce_predict(Z, Psi, coords, coef), cpu_reps)
            for v in des_ms.values():
                v["fraction_of_6.3TBps_of_the_store"] = P * C * size / (v["median_ms"] * 1e-3) / STREAM_BYTES_PER_S
            for ms in (des_ms, pre_ms):
                for v in ms.values():
                    v["G_factor_reads_per_s"] = P * C * N / (v["median_ms"] * 1e-3) / 1e9
            line = {"config": {"P": P, "N": N, "S": S, "C": C, "dtype": name, "reps": a.reps, "inner": a.inner, "cpu_reps": cpu_reps},
                    "design": {"store_bytes": P * C * size, "factor_reads": P * C * N, "ms": des_ms,
                               "largest_difference_to_torch": largest_difference(des_out["ttr_pce_design"], des_out["torch_gather_prod"]),
                               "largest_difference_to_cpu_mirror": largest_difference(des_out["ttr_pce_design"], cpu_M)},
                    "predict": {"factor_reads": P * C * N, "fmas": P * C, "ms": pre_ms,
                                "largest_difference_to_torch": largest_difference(pre_out["ttr_pce_predict"], pre_out["torch_gather_prod_matmul"]),
                                "largest_difference_to_cpu_mirror": largest_difference(pre_out["ttr_pce_predict"], cpu_y)}}
            lines.append(line)
            print(json.dumps(line), flush=True)
            del des_out, pre_out
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

"""``tn.convolve`` on one MI355X: the exact train from ``ttr_core_convolve`` (+ one ``round_tt``) next to the same cores built by
a torch composition on the device and by the CPU mirror.  Reads nothing but this package.

    python tools/convolve_bench.py                  # the three cases
    python tools/convolve_bench.py --only a --reps 20

Cases (cores are ``rand`` scaled by 2 / rank; modes of 64):
  a   6 modes, rank-16 fp32 field with a rank-1 9-tap kernel, 'same', no rounding (the ranks do not grow)
  b   6 modes, rank 16 with a rank-4 train of the same shape, 'full', rmax = 32, fp32
  c   as b in fp64 with 4 modes
Per case (ms, device events around work that ends in a synchronise; every variant warmed up once, the variants alternate inside
the repetition loop, the figure is the median of --reps; the three core-level variants run --inner times back to back inside
one timed window and are reported per build of the N cores):
  total            tn.convolve(t1, t2, ...) as a user calls it
  core_convolve    the N ttr_core_convolve launches alone (through the binding, output allocation included)
  round_tt         round_tt on a fresh copy of the exact train (b, c)
  torch_conv1d     the same N cores from torch.nn.functional.conv1d: a as [R1 R2, 1, I] signals, c as [S1 S2, 1, J] flipped
                   filters, the window cropped and the result permuted to [R1 S1, K, R2 S2]
  torch_toeplitz   the same N cores from one gather of c into a Toeplitz operand [S1, I, K, S2] (index and mask built outside
                   the timed region) and one einsum
  torch_best       the faster of the two;  ratio_torch_over_kernel = torch_best / core_convolve (>= 1: the kernel is not slower)
  cpu_mirror       _hostops.core_convolve on CPU copies of the cores (host clock, one repetition after a warm-up)
and the largest entry-wise difference between the kernel's and the compositions' cores relative to the largest entry.  Case a
also reports the bytes the N launches write over the core_convolve time as a fraction of 6.3 TB/s (the achievable HBM rate): at
these core sizes (64 KiB per core) that is a measure of launch overhead, not of the memory system.
One JSON line per case, appended to profiles/convolve_bench_mi355x.jsonl.
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
OUT = os.path.join(ROOT, "profiles", "convolve_bench_mi355x.jsonl")
HBM_ACHIEVABLE = 6.3e12


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
    for fn in fns.values():   # warm-up: code objects, allocator, library heuristics
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in fns.items():
            ms, last[k] = timed(fn)
            ts[k].append(ms)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ts.items()}, last


def conv1d_core(a, c, lo, K):
    (R1, I, R2), (S1, J, S2) = a.shape, c.shape
    x = a.permute(0, 2, 1).reshape(R1 * R2, 1, I)
    w = c.permute(0, 2, 1).reshape(S1 * S2, 1, J).flip(-1)
    y = torch.nn.functional.conv1d(x, w, padding=J - 1)[:, :, lo:lo + K]   # [R1 R2, S1 S2, K]: the full convolution, cropped
    return y.reshape(R1, R2, S1, S2, K).permute(0, 2, 4, 1, 3).reshape(R1 * S1, K, R2 * S2)


def toeplitz_plan(I, J, lo, K, device):
    idx = torch.arange(K, device=device)[None, :] + lo - torch.arange(I, device=device)[:, None]   # [I, K]: k + lo - i
    return idx.clamp(0, J - 1), (idx >= 0) & (idx < J)


def toeplitz_core(a, c, plan, K):
    (R1, I, R2), (S1, J, S2) = a.shape, c.shape
    idx, mask = plan
    Tc = c[:, idx, :] * mask[None, :, :, None].to(c.dtype)   # [S1, I, K, S2]
    return torch.einsum("aib,sikt->askbt", a, Tc).reshape(R1 * S1, K, R2 * S2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["a", "b", "c"], default=None)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10, help="back-to-back repetitions inside one timed window of the core-level variants")
    args = ap.parse_args()
    import tntorch_amd as tn
    from tntorch_amd import _hip, _hostops
    from tntorch_amd.tools import convolve_window

    if not torch.cuda.is_available():
        sys.exit("convolve_bench needs a GPU")
    dev = torch.device("cuda:0")
    I = args.size
    cases = {
        "a": dict(N=6, dtype=torch.float32, r1=16, r2=1, J=9, mode="same", kw=dict(eps=None)),
        "b": dict(N=6, dtype=torch.float32, r1=16, r2=4, J=I, mode="full", kw=dict(eps=None, rmax=32)),
        "c": dict(N=4, dtype=torch.float64, r1=16, r2=4, J=I, mode="full", kw=dict(eps=None, rmax=32)),
    }
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    for name, cfg in cases.items():
        if args.only not in (None, name):
            continue
        N, dt = cfg["N"], cfg["dtype"]
        t1, t2 = train(N, I, cfg["r1"], dt, dev), train(N, cfg["J"], cfg["r2"], dt, dev, seed=1)
        A, B = [c.contiguous() for c in t1.cores], [c.contiguous() for c in t2.cores]
        wins = [convolve_window(I, cfg["J"], cfg["mode"])] * N
        plans = [toeplitz_plan(I, cfg["J"], lo, K, dev) for lo, K in wins]

        def kernel():
            return [_hip.core_convolve(x, y, lo, K) for x, y, (lo, K) in zip(A, B, wins)]

        def repeated(fn):   # a timed window of `inner` builds of the N cores: longer than the clock's and the scheduler's grain
            def f():
                for _ in range(args.inner):
                    out = fn()
                return out
            return f

        exact = kernel()
        fns = {
            "total": lambda: tn.convolve(t1, t2, mode=cfg["mode"], **cfg["kw"]),
            "core_convolve": repeated(kernel),
            "torch_conv1d": repeated(lambda: [conv1d_core(x, y, lo, K) for x, y, (lo, K) in zip(A, B, wins)]),
            "torch_toeplitz": repeated(lambda: [toeplitz_core(x, y, p, K) for x, y, p, (lo, K) in zip(A, B, plans, wins)]),
        }
        if cfg["kw"].get("rmax") is not None:
            def rounding():
                t = tn.Tensor([c.clone() for c in exact])   # (the copies are inside the timed region: 2 MB per core)
                t.round_tt(eps=0, rmax=cfg["kw"]["rmax"])
                return t
            fns["round_tt"] = rounding
        ms, last = alternate(fns, args.reps)
        for k in ("core_convolve", "torch_conv1d", "torch_toeplitz"):   # per build of the N cores
            ms[k] = {q: v / args.inner for q, v in ms[k].items()}
        scale = max(float(c.abs().max()) for c in exact)
        diff = {k: max(float((x - y).abs().max()) for x, y in zip(last[k], exact)) / scale for k in ("torch_conv1d", "torch_toeplitz")}
        best = min(("torch_conv1d", "torch_toeplitz"), key=lambda k: ms[k]["median_ms"])
        Ah, Bh = [c.cpu() for c in A], [c.cpu() for c in B]
        mirror = lambda: [_hostops.core_convolve(x, y, lo, K) for x, y, (lo, K) in zip(Ah, Bh, wins)]  # noqa: E731
        mirror()
        t0 = time.perf_counter()
        mirror()
        cpu_ms = (time.perf_counter() - t0) * 1e3
        line = {"case": name, "config": {"modes": N, "size": I, "other_size": cfg["J"], "ranks": [cfg["r1"], cfg["r2"]],
                                         "dtype": str(dt), "mode": cfg["mode"], "rmax": cfg["kw"].get("rmax"), "reps": args.reps, "inner": args.inner},
                "ms": ms, "torch_best": best, "ratio_torch_over_kernel": ms[best]["median_ms"] / ms["core_convolve"]["median_ms"],
                "cpu_mirror_ms": cpu_ms, "largest_difference_over_largest_entry": diff,
                "ranks_exact": [1] + [int(c.shape[2]) for c in exact], "ranks_result": last["total"].ranks_tt.tolist()}
        if "round_tt" in ms:
            line["round_tt_share_of_total"] = ms["round_tt"]["median_ms"] / ms["total"]["median_ms"]
        if name == "a":
            written = sum(c.numel() * c.element_size() for c in exact)
            line["bytes_written"] = written
            line["fraction_of_achievable_hbm_on_bytes_written"] = written / (ms["core_convolve"]["median_ms"] * 1e-3) / HBM_ACHIEVABLE
        print(json.dumps(line), flush=True)
        with open(OUT, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

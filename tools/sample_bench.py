"""One mode of the sampling sweep (ttr_sample_step) on one MI355X next to the same step written with torch ops on the same GPU,
and a whole ``tn.sample``.

    python tools/sample_bench.py --out profiles/sample_bench_mi355x.jsonl
    python tools/sample_bench.py --shapes 65536x16x64 --dtypes f32           # one corner

Two kinds of JSON lines:

  "step"    P samples, a core [r, I, r] of normal entries, a non-negative fiber [r, I] and left rows, uniform thresholds: ms per call
              kernel   ``_hip.sample_step`` with a preallocated Lnew (one launch, nothing read back)
              torch    the reference's step restated with torch ops, also without a readback: the P x I matrix ``(L @ fiber).abs()``,
                       ``cumsum`` in fp64, a compare-and-count against u T, the gather of one core slice per sample and an ``einsum``
                       with it, the quotient by T.  (The slices are gathered as [P, r, r'], sample first: the reference's literal
                       ``core[:, x, :]`` [r, P, r'] sends torch's batched GEMM a leading dimension of P r', and at 2^32 elements that
                       route returned wrong values on the GPU this was written on.)
            ``flops`` = 2 P r I for q (the kernel forms q twice: ``kernel_flops`` = 4 P r I + 2 P r r), ``kernel_tflops`` =
            kernel_flops over the time (an achieved rate of what the kernel executes), ``matrix_bytes`` = the P x I matrix in the
            dtype, which the torch route writes and re-reads and the kernel never forms, ``same_x`` = the share of samples where
            both routes chose the same index and ``max_rel_diff`` the largest difference of the new left rows relative to the
            largest entry.
  "sample"  a whole ``tn.sample(t, P)`` on an N-mode train of rank R and mode size I (``rand`` cores): ms per call, host clock around a
            call that ends in the readback of the flag word; ``seed=None`` (thresholds drawn on the device) and ``seed=0`` (drawn
            on the host and uploaded).

Every "step" time is the best of --reps windows of --inner calls between two HIP events on the current stream (the window ends in
a synchronise), after one warm-up call per shape; the two routes alternate window by window.  Without a GPU the tool stops: it
never reports a CPU time as a device time.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def alternate(fns, reps, inner):
    """Best window of every variant (ms per call), the variants taking turns."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    best = {k: float("inf") for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            best[k] = min(best[k], window(fn, inner[k]))
    return best


def torch_step(L, fiber, core, u):
    """The reference's ``from_matrix`` and left update with torch ops on the device, decisions as in ttr_sample_step."""
    M = (L @ fiber).abs()
    c = torch.cumsum(M, dim=1, dtype=torch.float64)
    T = c[:, -1]
    x = (c <= (u * T)[:, None]).sum(dim=1).clamp_max(fiber.shape[1] - 1)
    G = core.permute(1, 0, 2).contiguous()[x]                     # [P, r, r']: one slice per sample
    Lnew = (torch.einsum("pa,pab->pb", L, G).double() / T[:, None]).to(L.dtype)
    return x, Lnew


def step_line(P, r, I, dtype, name, reps, inner):
    from tntorch_amd import _hip

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(P % 9973 + r + I)
    L = torch.rand((P, r), generator=g, dtype=dtype, device=dev)
    fiber = torch.rand((r, I), generator=g, dtype=dtype, device=dev)
    core = torch.randn((r, I, r), generator=g, dtype=dtype, device=dev)
    u = torch.rand((P,), generator=g, dtype=torch.float64, device=dev)
    X = torch.empty((P,), dtype=torch.int64, device=dev)
    Lnew = torch.empty((P, r), dtype=dtype, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    es = L.element_size()
    out = {"bench": "step", "P": P, "r": r, "I": I, "dtype": name, "reps": reps, "inner": inner, "flops": 2 * P * r * I,
           "kernel_flops": 4 * P * r * I + 2 * P * r * r, "matrix_bytes": P * I * es}
    _hip.sample_step(L, fiber, core, u, X, flag, Lnew)
    xt, Lt = torch_step(L, fiber, core, u)
    out["flag"] = int(flag.item())
    out["same_x"] = float((X == xt).double().mean())
    same = X == xt
    out["max_rel_diff"] = float(((Lnew[same] - Lt[same]).abs().max() / Lt[same].abs().max()))
    del xt, Lt
    ms = alternate({"kernel": lambda: _hip.sample_step(L, fiber, core, u, X, flag, Lnew), "torch": lambda: torch_step(L, fiber, core, u)},
                   reps, {"kernel": inner, "torch": max(1, inner // 5)})
    out["kernel_ms"], out["torch_ms"] = ms["kernel"], ms["torch"]
    out["kernel_tflops"] = out["kernel_flops"] / ms["kernel"] * 1e-9
    out["torch_over_kernel"] = ms["torch"] / ms["kernel"]
    return out


def sample_line(N, R, I, P, dtype, name, reps):
    import tntorch_amd as tn

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(N * 100 + R)
    rs = [1] + [R] * (N - 1) + [1]
    t = tn.Tensor([torch.rand(rs[n], I, rs[n + 1], generator=g, dtype=torch.float64).to(dtype).to(dev) for n in range(N)])
    out = {"bench": "sample", "N": N, "R": R, "I": I, "P": P, "dtype": name, "reps": reps}
    for key, seed in (("ms_seed_none", None), ("ms_seed_int", 0)):
        tn.sample(t, P, seed=seed)
        best = float("inf")
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tn.sample(t, P, seed=seed)          # (ends in the readback of the flag word)
            best = min(best, time.perf_counter() - t0)
        out[key] = best * 1e3
    out["samples_per_s"] = P / (out["ms_seed_none"] * 1e-3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["65536x16x64", "1048576x64x64", "1048576x64x512", "262144x128x4096"], help="PxrxI")
    ap.add_argument("--dtypes", nargs="+", default=["f32", "f64"], choices=["f32", "f64"])
    ap.add_argument("--modes", type=int, default=8)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sample_bench needs a GPU")
    sink = open(a.out, "a") if a.out else None

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if sink:
            sink.write(text + "\n")
            sink.flush()

    for name in a.dtypes:
        dtype = torch.float32 if name == "f32" else torch.float64
        for shp in a.shapes:
            P, r, I = (int(x) for x in shp.split("x"))
            emit(step_line(P, r, I, dtype, name, a.reps, a.inner))
        emit(sample_line(a.modes, a.rank, a.size, a.samples, dtype, name, a.reps))
    if sink:
        sink.close()


if __name__ == "__main__":
    main()

"""The minimisation step of TT-cross (ttr_minimize_step) on one MI355X next to the same step written with torch ops on the same
GPU, and a whole ``tn.minimum``.

    python tools/minimize_bench.py --out profiles/minimize_bench_mi355x.jsonl
    python tools/minimize_bench.py --blocks 64x512x64 --dtypes f32           # one corner

Two kinds of JSON lines:

  "step"     one fibre block (Ra, I, Rb) of random values with a state that already holds a best value: ms per call of
               kernel   ``_hip.minimize_step`` with a preallocated workspace (two launches, nothing read back)
               torch    the same step as torch ops, also without a readback: isfinite + all, a masked argmin of the original
                        values (where + argmin), the comparison with the state and the gathers of the position as 0-dim tensor
                        ops (torch.where on the state), then sub, atan, rsub on the block
             ``bytes`` = 2 M elements (the block read once and written once: what the step needs at least), ``kernel_gbs`` /
             ``torch_gbs`` = those bytes over the time (an achieved rate of the NEEDED traffic, not of the traffic a route
             really causes), and ``same_state``: both routes end in the same best value and position.
  "minimum"  a whole ``tn.minimum`` on an N-mode train of rank R and mode size I (``rand`` cores, scaled), default arguments:
             ms per call, host clock around a call that ends in the readback of the position.

Every "step" time is the best of --reps windows of --inner calls between two HIP events on the current stream (the window ends in
a synchronise), after one warm-up call per shape.  The step is in place and the calls of a window run on the block the call
before left: after one call every value lies in (0, pi), which is as good an input as the first.
Without a GPU the tool stops: it never reports a CPU time as a device time.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window_ms(fn, reps, inner):
    """Best of ``reps`` windows of ``inner`` calls, ms per call."""
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / inner)
    return best


def torch_step(e, Ra, I, Rb, lset, rset, best, pos, flags):
    """ttr_minimize_step's semantics with torch ops on the device, no readback (every decision is a torch.where)."""
    found = flags[0] != 0
    m0 = torch.where(found, best[0], torch.zeros((), dtype=e.dtype, device=e.device))
    fin = torch.isfinite(e)
    clean = fin.all()
    m = torch.argmin(torch.where(fin, e, torch.full((), math.inf, dtype=e.dtype, device=e.device)))
    v = e[m]
    take = clean & (~found | (v < best[0]))
    c, ai = m % Rb, m // Rb
    new_pos = torch.cat([lset[ai // I, 1:], (ai % I)[None], rset[c, : rset.shape[1] - 1]])
    best.copy_(torch.where(take, v, best[0])[None])
    pos.copy_(torch.where(take, new_pos, pos))
    flags.copy_(torch.stack([(found | take).int(), (flags[1] != 0).int() | (~clean).int()]))
    e.sub_(m0).atan_().neg_().add_(math.pi / 2)
    return e


def step_line(Ra, I, Rb, dtype, name, reps, inner):
    from tntorch_amd import _hip

    dev = torch.device("cuda:0")
    M = Ra * I * Rb
    g = torch.Generator().manual_seed(M % 9973)
    src = torch.randn(M, generator=g, dtype=torch.float32).to(dtype).to(dev)
    nl, nr = 3, 4
    lset = torch.randint(0, 64, (Ra, nl + 1), generator=g).to(dev)
    rset = torch.randint(0, 64, (Rb, nr + 1), generator=g).to(dev)
    ws = torch.empty(_hip.minimize_workspace_bytes(dtype, M), dtype=torch.uint8, device=dev)

    def fresh():
        return (torch.full((1,), 10.0, dtype=dtype, device=dev), torch.zeros(nl + 1 + nr, dtype=torch.int64, device=dev),
                torch.tensor([1, 0], dtype=torch.int32, device=dev))

    out = {"bench": "step", "Ra": Ra, "I": I, "Rb": Rb, "dtype": name, "reps": reps, "inner": inner,
           "bytes": 2 * M * src.element_size()}
    sk, st = fresh(), fresh()
    ek, et = src.clone(), src.clone()
    _hip.minimize_step(ek, Ra, I, Rb, lset, rset, *sk, workspace=ws)
    torch_step(et, Ra, I, Rb, lset, rset, *st)
    out["same_state"] = bool(torch.equal(sk[0], st[0]) and torch.equal(sk[1], st[1]) and torch.equal(sk[2], st[2]))
    out["max_abs_diff"] = float((ek - et).abs().max())
    out["kernel_ms"] = window_ms(lambda: _hip.minimize_step(ek, Ra, I, Rb, lset, rset, *sk, workspace=ws), reps, inner)
    out["torch_ms"] = window_ms(lambda: torch_step(et, Ra, I, Rb, lset, rset, *st), reps, inner)
    out["kernel_gbs"] = out["bytes"] / out["kernel_ms"] * 1e-6
    out["torch_gbs"] = out["bytes"] / out["torch_ms"] * 1e-6
    return out


def minimum_line(N, R, I, dtype, name, reps):
    import tntorch_amd as tn

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(N * 100 + R)
    rs = [1] + [R] * (N - 1) + [1]
    t = tn.Tensor([((torch.rand(rs[n], I, rs[n + 1], generator=g, dtype=torch.float64) - 0.3) * (2.0 / R)).to(dtype).to(dev) for n in range(N)])

    def call():
        torch.manual_seed(0)
        np.random.seed(0)
        return tn.argmin(t)

    pos = call()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()                      # (ends in the readback of the position)
        best = min(best, time.perf_counter() - t0)
    torch.manual_seed(0)
    np.random.seed(0)
    return {"bench": "minimum", "N": N, "R": R, "I": I, "dtype": name, "reps": reps, "ms": best * 1e3, "argmin": list(pos),
            "minimum": float(tn.minimum(t))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", nargs="+", default=["16x64x16", "64x512x64", "128x4096x128"], help="RaxIxRb")
    ap.add_argument("--dtypes", nargs="+", default=["f32", "f64"], choices=["f32", "f64"])
    ap.add_argument("--modes", type=int, default=8)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("minimize_bench needs a GPU")
    sink = open(a.out, "a") if a.out else None

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if sink:
            sink.write(text + "\n")
            sink.flush()

    for name in a.dtypes:
        dtype = torch.float32 if name == "f32" else torch.float64
        for blk in a.blocks:
            Ra, I, Rb = (int(x) for x in blk.split("x"))
            emit(step_line(Ra, I, Rb, dtype, name, a.reps, a.inner))
        emit(minimum_line(a.modes, a.rank, a.size, dtype, name, a.reps))
    if sink:
        sink.close()


if __name__ == "__main__":
    main()

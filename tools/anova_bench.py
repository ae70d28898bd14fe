"""Sobol indices of a tensor train (tn.sobol) on one MI355X: the fused sandwich kernel next to the two routes it replaces.

    python tools/anova_bench.py --out profiles/anova_bench_mi355x.jsonl
    python tools/anova_bench.py --sizes 64 --ranks 16 --dtypes f32          # one corner

The train has N modes of size I with ``rand`` cores scaled by 2 / rank and random positive marginals.  Two kinds of JSON lines:

  "mode"    one interior mode, Z [S, R, R] random, A [R, I, R], w, mu = the weighted mean: ms per call of
              fused       one ttr_mode_sandwich launch plus the reduction of its partials (``_hip.mode_sandwich``)
              hsum        S ttr_hsum_step(K = 3) calls on a centred copy of the core (``_hipops.mode_sandwich_hsum``: the route
                          above the fused kernel's rank limit), the copy included
              ref_step    the step the reference's algorithm takes at this mode: one step of ``dot(a, mask(am, m))``, the two GEMMs
                          of ``_hipops.dot`` on the extended core [R, I + 1, R] and the masked, weighted one [R S, I + 1, R S]
                          (mask core: ``weight_one_hot`` with rank S), interface [R S, R]; ``ref_build`` is the core_kron that
                          builds the masked core.  It yields one number per mode and mask where the other two yield Q for S
                          interfaces, so it is a cost of the same job, not the same arithmetic.
            plus ``traffic``: the bytes each route moves through memory at least once, counted from the shapes, and
            ``max_rel_diff``: fused against hsum, relative to the largest entry.
  "sobol"   the whole ``tn.sobol(t, tn.weight_one_hot(N))``: ms per call with the fused kernel and with
            ``_hipops.SANDWICH_FUSED_MAX_RANK = 0`` (every step on the hsum route), and the largest difference of the indices.

Every time is the best of --reps windows of --inner calls between two HIP events on the current stream (the window ends in a
synchronise), after one warm-up call per shape.  Without a GPU the tool stops: it never reports a CPU time as a device time.
"""
import argparse
import json
import os
import sys

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


def train(N, I, r, dtype, device, seed=0):
    import tntorch_amd as tn

    g = torch.Generator().manual_seed(seed)
    rs = [1] + [r] * (N - 1) + [1]
    cores = [(torch.rand(rs[n], I, rs[n + 1], generator=g, dtype=torch.float64) * (2.0 / r)).to(dtype).to(device) for n in range(N)]
    marg = [(torch.rand(I, generator=g, dtype=torch.float64) + 0.1).to(dtype).to(device) for _ in range(N)]
    return tn.Tensor(cores), marg


def mode_line(S, R, I, dtype, name, reps, inner):
    import tntorch_amd as tn
    from tntorch_amd import _hip, _hipops

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(S * 1000 + R)
    Z = torch.randn(S, R, R, generator=g, dtype=torch.float64).to(dtype).to(dev)
    A = (torch.rand(R, I, R, generator=g, dtype=torch.float64) * (2.0 / R)).to(dtype).to(dev)
    w = torch.rand(I, generator=g, dtype=torch.float64) + 0.1
    w = (w / w.sum()).to(dtype).to(dev)
    mu = _hipops.mode_reduce(A, w)
    el = 4 if dtype == torch.float32 else 8
    out = {"bench": "mode", "S": S, "R": R, "I": I, "dtype": name, "reps": reps, "inner": inner}
    fused = _hip.mode_sandwich(Z, A, w, mu)
    hsum = _hipops.mode_sandwich_hsum(Z, A, w, mu)
    out["max_rel_diff"] = float((fused - hsum).abs().max() / hsum.abs().max())
    out["fused_ms"] = window_ms(lambda: _hip.mode_sandwich(Z, A, w, mu), reps, inner)
    out["hsum_ms"] = window_ms(lambda: _hipops.mode_sandwich_hsum(Z, A, w, mu), reps, inner)
    # the reference's algorithm at this mode: extended cores and one step of the dot
    ext = torch.cat([mu[:, None, :], A - mu[:, None, :]], dim=1).contiguous()                       # [R, I + 1, R]
    extw = torch.cat([mu[:, None, :], (A - mu[:, None, :]) * w[None, :, None]], dim=1).contiguous()
    mcore = (tn.weight_one_hot(3, S, dtype=dtype, device=dev).cores[1] if S > 1 else torch.ones(1, 2, 1, dtype=dtype, device=dev))
    idx = torch.tensor([0] + [1] * I, device=dev)
    msel = mcore[:, idx, :].contiguous()                                                            # [S, I + 1, S]

    def build():
        return _hipops.core_kron(extw[None], msel[None])                                            # [1, R S, I + 1, R S]

    masked = build()
    L = torch.randn(1, R * S, R, generator=g, dtype=torch.float64).to(dtype).to(dev)

    def step():
        U = _hip.gemm(L, ext.reshape(1, R, (I + 1) * R)).reshape(1, R * S * (I + 1), R)
        return _hip.gemm(masked.reshape(1, R * S * (I + 1), R * S), U, transA=True)

    out["ref_build_ms"] = window_ms(build, reps, inner)
    out["ref_step_ms"] = window_ms(step, reps, inner)
    nsplit_bytes = max(_hip.mode_sandwich_workspace_bytes(dtype, S, R, I, R), 0)
    out["traffic"] = {
        "core_bytes": R * I * R * el,
        "fused_bytes": (R * I * R + 2 * S * R * R + R * R) * el + 2 * nsplit_bytes,
        "hsum_bytes": (2 * R * I * R + S * (6 * R * I * R + 2 * R * R)) * el,
        "ref_step_bytes": ((I + 1) * R * R * (1 + S * S) + 2 * S * (I + 1) * R * R + 2 * S * R * R) * el,
    }
    return out


def sobol_line(N, R, I, dtype, name, reps):
    import tntorch_amd as tn
    from tntorch_amd import _hipops

    dev = torch.device("cuda:0")
    t, marg = train(N, I, R, dtype, dev)
    mask = tn.weight_one_hot(N, dtype=dtype, device=dev)
    fn = lambda: tn.sobol(t, mask, marg)  # noqa: E731
    out = {"bench": "sobol", "N": N, "R": R, "I": I, "dtype": name, "mask": "weight_one_hot", "reps": reps}
    saved = _hipops.SANDWICH_FUSED_MAX_RANK
    try:
        fused = fn().torch()
        out["fused_ms"] = window_ms(fn, reps, 1)
        _hipops.SANDWICH_FUSED_MAX_RANK = 0
        hsum = fn().torch()
        out["hsum_ms"] = window_ms(fn, reps, 1)
    finally:
        _hipops.SANDWICH_FUSED_MAX_RANK = saved
    out["max_abs_diff"] = float((fused - hsum).abs().max())
    out["indices_sum"] = float(fused.sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", type=int, default=8)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--ranks", type=int, nargs="+", default=[16, 32, 64])
    ap.add_argument("--stacks", type=int, nargs="+", default=[1, 9], help="S: interfaces per launch")
    ap.add_argument("--dtypes", nargs="+", default=["f32", "f64"], choices=["f32", "f64"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("anova_bench needs a GPU")
    sink = open(a.out, "a") if a.out else None

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if sink:
            sink.write(text + "\n")
            sink.flush()

    for name in a.dtypes:
        dtype = torch.float32 if name == "f32" else torch.float64
        for I in a.sizes:
            for R in a.ranks:
                for S in a.stacks:
                    emit(mode_line(S, R, I, dtype, name, a.reps, a.inner))
                emit(sobol_line(a.modes, R, I, dtype, name, a.reps))
    if sink:
        sink.close()


if __name__ == "__main__":
    main()

"""Point evaluation t[idx] on the device (ttr_gather_chain), against a byte model and against the reference's algorithm.

    python tools/index_bench.py [--reps 10] [--direct-sweep]

Cases: 2^20 random points on one 64^8 rank-64 fp32 train; B = 64 such trains x 2^14 points; P = 1 and P = 256.  Reported per
case: ms per call (HIP events, median of --reps after one untimed call), points/s, and the byte model's floor as a fraction of
the measured time.  The byte model counts what the chain must move: the running product X written once per mode and read once
per later mode (P * r_a * r rows), one read of each index column per pass (validate, histogram, scatter, step), the permutation
written and read once per sorted mode, and the cores once; at 6.0 TB/s (MI355X_MICROARCH.md: rows gathered from a table swept
out of HBM), since X (256 MB at 2^20 points) does not stay in the Infinity Cache.

For comparison the same query through the reference's algorithm (tensor.py:1357-1378: per mode, gather the [r, P, r'] slices
and contract with torch.einsum) on the same device, in chunks of 2^16 points (one gathered 64^8 rank-64 mode at 2^20 points is
16 GB).  --direct-sweep times the direct path (one tile per point) against the sorted path for small P: the threshold in
ttr_index.hip (kDefaultDirectMax) comes from it.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.0


def make_train(B, N, I, R, dtype, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    ranks = [1] + [R] * (N - 1) + [1]
    return [torch.randn(B, ranks[n], I, ranks[n + 1], generator=g, device=dev, dtype=dtype) / ranks[n] ** 0.5 for n in range(N)]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def model_bytes(B, N, I, R, P, es, sorted_path):
    ranks = [1] + [R] * (N - 1) + [1]
    x = 0
    for n in range(N):
        x += B * P * ranks[0] * ranks[n + 1] * es  # written by mode n
        if n > 0:
            x += B * P * ranks[0] * ranks[n] * es  # read by mode n
    passes = 4 if sorted_path else 2
    idx = N * P * 8 * passes + (N - 1) * P * 8 * 2 * (1 if sorted_path else 0)
    cores = B * sum(ranks[n] * I * ranks[n + 1] for n in range(N)) * es
    return x + idx + cores


def reference_einsum(cores, cols, chunk=1 << 16):
    """tensor.py:1357-1378 for a whole-train index block (non-batch): gathered slices, one einsum per mode."""
    P = cols[0].shape[0]
    outs = []
    for s in range(0, P, chunk):
        sl = [c[s:s + chunk] for c in cols]
        X = cores[0][0][:, sl[0], :]
        for c, i in zip(cores[1:], sl[1:]):
            X = torch.einsum("iaj,jak->iak", X, c[0][:, i, :])
        outs.append(X)
    return torch.cat(outs, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--direct-sweep", action="store_true")
    ap.add_argument("--only", default="", help="comma list of case names")
    ap.add_argument("--no-reference", action="store_true")
    a = ap.parse_args()

    import __graft_entry__ as g

    g.build()
    import tntorch_amd as tn
    from tntorch_amd import _hip

    dev = torch.device("cuda:0")
    N, I, R = 8, 64, 64
    cases = [("p2^20", 1, 1 << 20), ("b64_p2^14", 64, 1 << 14), ("p1", 1, 1), ("p256", 1, 256)]
    if a.only:
        cases = [c for c in cases if c[0] in a.only.split(",")]
    results = []
    for name, B, P in cases:
        cores = make_train(B, N, I, R, torch.float32, dev)
        t = tn.Tensor(cores if B > 1 else [c[0] for c in cores], batch=B > 1)
        gi = torch.Generator(device=dev).manual_seed(1)
        idx = torch.randint(0, I, (P, N), generator=gi, device=dev)
        key = idx if B == 1 else (slice(None),) + tuple(idx[:, n] for n in range(N))
        ms = timed(lambda: t[key], a.reps)
        sorted_path = P > 1024
        mb = model_bytes(B, N, I, R, P, 4, sorted_path)
        floor_ms = mb / (HBM_TBS * 1e12) * 1e3
        res = {"case": name, "B": B, "P": P, "ms": round(ms, 4), "points_per_s": B * P / (ms * 1e-3),
               "model_GB": round(mb / 1e9, 4), "floor_ms": round(floor_ms, 4), "floor_fraction": round(floor_ms / ms, 3)}
        if B == 1 and not a.no_reference:
            cols = [idx[:, n] for n in range(N)]
            ref_ms = timed(lambda: reference_einsum(cores, cols), max(2, a.reps // 3))
            ours = t[idx].cores[0].reshape(-1).double()
            ref = reference_einsum(cores, cols).reshape(-1).double()
            res["reference_einsum_ms"] = round(ref_ms, 4)
            res["speedup_vs_reference"] = round(ref_ms / ms, 2)
            res["rel_diff_vs_reference"] = float((ours - ref).norm() / ref.norm())
        results.append(res)
        print(json.dumps(res), flush=True)
        del t, cores
        torch.cuda.empty_cache()

    if a.direct_sweep:
        cores = make_train(1, N, I, R, torch.float32, dev)
        for P in (1, 16, 64, 256, 1024, 4096):
            cols = [torch.randint(0, I, (P,), device=dev) for _ in range(N)]
            d = timed(lambda: _hip.gather_chain(cores, cols, direct_max_points=1 << 40), a.reps)
            s = timed(lambda: _hip.gather_chain(cores, cols, direct_max_points=0), a.reps)
            print(json.dumps({"sweep_P": P, "direct_ms": round(d, 4), "sorted_ms": round(s, 4)}), flush=True)


if __name__ == "__main__":
    main()

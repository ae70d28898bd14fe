"""The core gradient of the differentiable point evaluation (ttr_gather_grad) on one MI355X next to the same step written with torch
ops on the same GPU, and one whole forward + backward of ``t[X]``.

    python tools/autodiff_bench.py --out profiles/autodiff_bench_mi355x.jsonl
    python tools/autodiff_bench.py --shapes 1048576x16x16x64 --dtypes f32        # one corner

Two kinds of JSON lines:

  "grad"   P samples spread uniformly over I slices, left rows L [P, r0] and right rows R [P, r1] of normal entries, the grouping
           plan built beforehand (it is cached across the iterations of a fit): ms per call
              kernel   ``_hipops.gather_grad`` (two launches, the workspace allocated per call as the backward does)
              torch    ``index_add_`` of the broadcast product L[:, :, None] * R[:, None, :] into a zero [I, r0, r1] tensor, in chunks
                       of at most --chunk-bytes of outer products (``torch_chunks`` of them)
           ``flops`` = 2 P r0 r1, ``kernel_tflops`` the achieved rate, ``read_bytes`` = P (r0 + r1) elements (what the kernel reads
           once per 64-column tile of the other side), ``outer_bytes`` = P r0 r1 elements, which the torch route writes and re-reads
           and the kernel never forms; ``max_rel_diff`` the largest difference of the two results relative to the largest entry.
  "fit"    forward + backward of ``(t[X].torch() ** 2).sum()`` on an N-mode train of rank R and mode size I at P points: ms per call
              ours     the autograd Function (N gather steps forward; N gather_grad and N - 1 gather steps backward)
              torch    the reference's route under torch autograd: gathered slices ``core[:, X[:, n], :]`` and an einsum chain

Every time is the best of --reps windows of --inner calls between two HIP events on the current stream (the window ends in a
synchronise), after one warm-up call per variant; the variants alternate window by window.  Without a GPU the tool stops: it never
reports a CPU time as a device time.
"""
import argparse
import json
import os
import sys

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


def torch_grad(L, R, col, I, chunk):
    dG = torch.zeros((I, L.shape[1], R.shape[1]), dtype=L.dtype, device=L.device)
    for p0 in range(0, L.shape[0], chunk):
        p1 = min(p0 + chunk, L.shape[0])
        dG.index_add_(0, col[p0:p1], L[p0:p1, :, None] * R[p0:p1, None, :])
    return dG.permute(1, 0, 2)


def grad_line(P, r0, r1, I, dtype, name, reps, inner, chunk_bytes):
    from tntorch_amd import _hipops, autodiff

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(P % 9973 + r0 + r1 + I)
    L = torch.randn((P, r0), generator=g, dtype=dtype, device=dev)
    R = torch.randn((P, r1), generator=g, dtype=dtype, device=dev)
    col = torch.randint(0, I, (P,), generator=g, device=dev)
    perm, plan = autodiff.build_plan(col, I)
    es = L.element_size()
    chunk = max(1, min(P, chunk_bytes // (r0 * r1 * es)))
    out = {"bench": "grad", "P": P, "r0": r0, "r1": r1, "I": I, "dtype": name, "reps": reps, "inner": inner, "ntasks": plan.ntasks,
           "flops": 2 * P * r0 * r1, "read_bytes": P * (r0 + r1) * es, "outer_bytes": P * r0 * r1 * es, "torch_chunks": -(-P // chunk)}
    a = _hipops.gather_grad(L, R, perm, plan)
    b = torch_grad(L, R, col, I, chunk)
    out["max_rel_diff"] = float((a - b).abs().max() / b.abs().max())
    del a, b
    ms = alternate({"kernel": lambda: _hipops.gather_grad(L, R, perm, plan), "torch": lambda: torch_grad(L, R, col, I, chunk)},
                   reps, {"kernel": inner, "torch": max(1, inner // 5)})
    out["kernel_ms"], out["torch_ms"] = ms["kernel"], ms["torch"]
    out["kernel_tflops"] = out["flops"] / ms["kernel"] * 1e-9
    out["torch_over_kernel"] = ms["torch"] / ms["kernel"]
    return out


def fit_line(N, R, I, P, dtype, name, reps, inner):
    import tntorch_amd as tn

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(N * 100 + R)
    rs = [1] + [R] * (N - 1) + [1]
    cores = [(torch.randn(rs[n], I, rs[n + 1], generator=g, dtype=torch.float64) / R ** 0.5).to(dtype).to(dev).requires_grad_()
             for n in range(N)]
    t = tn.Tensor(cores)
    X = torch.randint(0, I, (P, N), generator=g).to(dev)

    def ours():
        for c in cores:
            c.grad = None
        (t[X].torch() ** 2).sum().backward()

    def ref():
        for c in cores:
            c.grad = None
        v = cores[0][:, X[:, 0], :]
        for n in range(1, N):
            v = torch.einsum("ipj,jpk->ipk", v, cores[n][:, X[:, n], :])
        (v ** 2).sum().backward()

    out = {"bench": "fit", "N": N, "R": R, "I": I, "P": P, "dtype": name, "reps": reps, "inner": inner,
           "saved_bytes": P * sum(rs[:N]) * cores[0].element_size()}
    ours()
    mine = [c.grad.clone() for c in cores]
    ref()
    out["max_rel_diff"] = max(float((a - c.grad).abs().max() / c.grad.abs().max()) for a, c in zip(mine, cores))
    del mine
    ms = alternate({"ours": ours, "torch": ref}, reps, {"ours": inner, "torch": inner})
    out["ours_ms"], out["torch_ms"] = ms["ours"], ms["torch"]
    out["torch_over_ours"] = ms["torch"] / ms["ours"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1048576x16x16x64", "1048576x64x64x512", "262144x128x128x4096", "1048576x1x64x512"],
                    help="Pxr0xr1xI")
    ap.add_argument("--dtypes", nargs="+", default=["f32", "f64"], choices=["f32", "f64"])
    ap.add_argument("--modes", type=int, default=8)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--chunk-bytes", type=int, default=1 << 30)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("autodiff_bench needs a GPU")
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
            P, r0, r1, I = (int(x) for x in shp.split("x"))
            emit(grad_line(P, r0, r1, I, dtype, name, a.reps, a.inner, a.chunk_bytes))
        emit(fit_line(a.modes, a.rank, a.size, a.samples, dtype, name, a.reps, max(1, a.inner // 5)))
    if sink:
        sink.close()


if __name__ == "__main__":
    main()

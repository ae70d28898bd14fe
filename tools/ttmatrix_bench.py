"""The product of a TT-matrix / CP-matrix with a dense batch on one MI355X: single steps (ttr_ttm_step) next to the reference's own
einsum for that step on the same GPU, and whole ``tn.tt_multiply`` / ``tn.cp_multiply`` next to the reference's chain written with
torch ops and next to the dense product ``x @ M``.

    python tools/ttmatrix_bench.py --out profiles/ttmatrix_bench_mi355x.jsonl
    python tools/ttmatrix_bench.py --layers 4,8,8,4:16:256 --dtypes f32          # one corner

A layer is ``i_0,..,i_{d-1}:rank:batch`` (output modes = input modes, every inner TT rank = rank, CP rank = rank).  Two kinds of
JSON lines, each for fp32 and fp64:

  "step"      the first, a middle and the last step of a layer: X [I, D, R] random, G [R, I, O, S] random.  ms per call
                kernel   ``_hip.ttm_step`` into a preallocated Y (one launch)
                einsum   ``torch.einsum("idr,riob->dob", X, G)``: the reference's call for that step (matrix.py:435, 441)
              ``flops`` = 2 D (I R) (O S), ``bytes`` = the elements of X, G and Y once, in the dtype; ``kernel_tflops`` / ``kernel_tbs``
              and ``einsum_tflops`` / ``einsum_tbs`` = those over the time: achieved rates of what the algorithm needs, not counters;
              ``max_err_over_bound``: the kernel against the einsum in units of the step bound 2 (K + 1) u |X| . |G|.
  "multiply"  a whole product of a batch [b, rows]: ms per call
                tt_multiply / cp_multiply   the package (d launches; cp: + the sum over the rank)
                tt_chain / cp_chain         the reference's functions restated with torch ops on the device (transpose, reshape,
                                            one einsum per core)
                dense                       ``x @ M`` with M precomputed, where M has at most --dense-limit elements (a TT layer
                                            is NOT a faster dense layer at these sizes unless this line says so); null otherwise
              ``dense_elements`` = rows cols, ``tt_parameters`` / ``cp_parameters`` = the elements of the cores.

Every time is the best of --reps windows of --inner calls between two HIP events on the current stream (the window ends in a
synchronise), after one warm-up call per shape and route; the routes alternate window by window.  Without a GPU the tool stops:
it never reports a CPU time as a device time.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT_LAYERS = ["4,8,8,4:8:256", "4,8,8,4:16:256", "4,8,8,4:32:256", "4,8,8,4:8:4096", "4,8,8,4:16:4096", "4,8,8,4:32:4096",
                  "8,8,8,8:16:1024", "16,16,16,16:8:64"]


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
    """Best window of every route (ms per call), the routes taking turns."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    best = {k: float("inf") for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            best[k] = min(best[k], window(fn, inner))
    return best


def tt_chain(cores, x2d):
    """matrix.py:420-443 with torch ops."""
    b = x2d.shape[0]
    res = x2d.t().reshape(cores[0].shape[1], -1)
    res = torch.einsum("id,lior->ldor", res, cores[0])
    for G in cores[1:]:
        res = torch.einsum("idr,riob->dob", res.reshape(G.shape[1], -1, G.shape[0]), G)
    return res.reshape(b, -1)


def cp_chain(cores, x2d):
    """matrix.py:446-468 with torch ops."""
    b = x2d.shape[0]
    res = x2d.t().reshape(cores[0].shape[0], -1)
    res = torch.einsum("ij,ior->jor", res, cores[0])
    for C in cores[1:]:
        res = torch.einsum("ior,idr->dor", C, res.reshape(C.shape[0], -1, C.shape[-1]))
    return res.sum(-1).reshape(b, -1)


def step_shapes(dims, rank, batch):
    """(which, I, D, R, O, S) of the first, a middle and the last step of the layer."""
    d = len(dims)
    rows = 1
    for n in dims:
        rows *= n
    rk = [1] + [rank] * (d - 1) + [1]
    out = []
    for which, k in (("first", 0), ("middle", d // 2), ("last", d - 1)):
        D = batch * rows // dims[k]          # (I_{k+1} .. I_{d-1}, b, O_0 .. O_{k-1}) with O = I
        out.append((which, dims[k], D, rk[k], dims[k], rk[k + 1]))
    return out


def step_line(layer, which, I, D, R, O, S, dtype, name, reps, inner):
    from tntorch_amd import _hip

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(I + 7 * R + 13 * S)
    X = torch.randn((I, D, R), generator=g, dtype=dtype, device=dev)
    G = torch.randn((R, I, O, S), generator=g, dtype=dtype, device=dev)
    Y = torch.empty((D, O, S), dtype=dtype, device=dev)
    es = X.element_size()
    out = {"bench": "step", "layer": layer, "step": which, "I": I, "D": D, "R": R, "O": O, "S": S, "dtype": name, "reps": reps, "inner": inner,
           "flops": 2 * D * I * R * O * S, "bytes": (X.numel() + G.numel() + Y.numel()) * es}
    _hip.ttm_step(X, G, out=Y)
    ref = torch.einsum("idr,riob->dob", X, G)
    mag = torch.einsum("idr,riob->dob", X.abs(), G.abs())
    u = 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53
    out["max_err_over_bound"] = float(((Y - ref).abs().double() / (2 * (I * R + 1) * u * mag.double())).max())
    del ref, mag
    ms = alternate({"kernel": lambda: _hip.ttm_step(X, G, out=Y), "einsum": lambda: torch.einsum("idr,riob->dob", X, G)}, reps, inner)
    for k in ("kernel", "einsum"):
        out[k + "_ms"] = ms[k]
        out[k + "_tflops"] = out["flops"] / ms[k] * 1e-9
        out[k + "_tbs"] = out["bytes"] / ms[k] * 1e-9
    out["einsum_over_kernel"] = ms["einsum"] / ms["kernel"]
    return out


def multiply_line(layer, dims, rank, batch, dtype, name, reps, inner, dense_limit):
    import tntorch_amd as tn

    dev = torch.device("cuda:0")
    d = len(dims)
    g = torch.Generator(device=dev).manual_seed(rank + batch)
    rk = [1] + [rank] * (d - 1) + [1]
    scale = [1.0 / (dims[k] * rk[k]) ** 0.5 for k in range(d)]       # keeps the product's entries of order 1
    tt = [torch.randn((rk[k], dims[k], dims[k], rk[k + 1]), generator=g, dtype=dtype, device=dev) * scale[k] for k in range(d)]
    cp = [torch.randn((dims[k], dims[k], rank), generator=g, dtype=dtype, device=dev) / dims[k] ** 0.5 for k in range(d)]
    ttm, cpm = tn.TTMatrix(tt, None, dims, dims), tn.CPMatrix(cp, None, dims, dims)
    rows = 1
    for n in dims:
        rows *= n
    x = torch.randn((batch, rows), generator=g, dtype=dtype, device=dev)
    out = {"bench": "multiply", "layer": layer, "dims": dims, "rank": rank, "batch": batch, "dtype": name, "reps": reps, "inner": inner,
           "dense_elements": rows * rows, "tt_parameters": sum(c.numel() for c in tt), "cp_parameters": sum(c.numel() for c in cp)}
    y, yc = tn.tt_multiply(ttm, x), tt_chain(tt, x)
    out["tt_max_rel_diff"] = float((y - yc).abs().max() / yc.abs().max())
    z, zc = tn.cp_multiply(cpm, x), cp_chain(cp, x)
    out["cp_max_rel_diff"] = float((z - zc).abs().max() / zc.abs().max())
    del y, yc, z, zc
    fns = {"tt_multiply": lambda: tn.tt_multiply(ttm, x), "tt_chain": lambda: tt_chain(tt, x),
           "cp_multiply": lambda: tn.cp_multiply(cpm, x), "cp_chain": lambda: cp_chain(cp, x)}
    if rows * rows <= dense_limit:
        M = ttm.torch()
        fns["dense"] = lambda: x @ M
    ms = alternate(fns, reps, inner)
    for k in ("tt_multiply", "tt_chain", "cp_multiply", "cp_chain", "dense"):
        out[k + "_ms"] = ms.get(k)
    out["tt_chain_over_tt_multiply"] = ms["tt_chain"] / ms["tt_multiply"]
    out["cp_chain_over_cp_multiply"] = ms["cp_chain"] / ms["cp_multiply"]
    out["dense_over_tt_multiply"] = ms["dense"] / ms["tt_multiply"] if "dense" in ms else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", nargs="+", default=DEFAULT_LAYERS, help="i_0,..,i_{d-1}:rank:batch")
    ap.add_argument("--dtypes", nargs="+", default=["f32", "f64"], choices=["f32", "f64"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--dense-limit", type=int, default=1 << 28, help="largest dense matrix (elements) the dense comparator forms")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ttmatrix_bench needs a GPU")
    sink = open(a.out, "a") if a.out else None

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if sink:
            sink.write(text + "\n")
            sink.flush()

    for name in a.dtypes:
        dtype = torch.float32 if name == "f32" else torch.float64
        for layer in a.layers:
            dims, rank, batch = layer.split(":")
            dims, rank, batch = [int(v) for v in dims.split(",")], int(rank), int(batch)
            for which, I, D, R, O, S in step_shapes(dims, rank, batch):
                emit(step_line(layer, which, I, D, R, O, S, dtype, name, a.reps, a.inner))
            emit(multiply_line(layer, dims, rank, batch, dtype, name, a.reps, a.inner, a.dense_limit))
    if sink:
        sink.close()


if __name__ == "__main__":
    main()

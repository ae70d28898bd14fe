"""Rows of a TT-matrix (``tn.tt_lookup``, the TT embedding table) on one MI355X: one step (ttr_ttm_lookup_step) next to the same
step written with torch ops on the same GPU, and the whole lookup next to the chain in torch ops, next to ``index_select`` on the
dense matrix and next to ``tn.tt_multiply`` on a one-hot batch.

    python tools/lookup_bench.py --out profiles/lookup_bench_mi355x.jsonl
    python tools/lookup_bench.py --tables 16,16,16,16:4,4,4,4:16 --samples 4096 --dtypes f32          # one corner

A table is ``i_1,..,i_d:o_1,..,o_d:rank`` (every inner TT rank = rank); the rows are drawn uniformly.  Two kinds of JSON lines,
each for fp32 and fp64 and every P of --samples:

  "step"    the second core's step: X = G_1 viewed [I_1, O_1, r] read through the row map i_1 (the chain's first launch), G_2
            [r, I_2, O_2, r'].  ms per call
              kernel   ``_hip.ttm_lookup_step`` into a preallocated Y with a preallocated workspace (validation, the counting
                       sort and the GEMM launch: everything the entry enqueues)
              torch    ``torch.bmm`` of the gathered rows [P, D, R] with the gathered slices [P, R, O S], in chunks of samples
                       whose gathered slices stay below --gather-limit bytes
            ``flops`` = 2 P D R O S; ``bytes`` = the gathered X rows, the core and Y once, in the dtype; ``kernel_tflops`` /
            ``kernel_tbs`` = those over the time: achieved rates of what the algorithm needs, not counters;
            ``max_err_over_bound``: the kernel against the torch route in units of the step bound 2 (R + 1) u |X| . |G|
            (P <= 2^16; null above).
  "lookup"  the whole call, rows [P] -> [P, cols]: ms per call
              tt_lookup   the package (the digit table, d - 1 launches, one readback of the flag word)
              chain       the same chain in torch ops (gathered slices + bmm, chunked as above)
              dense       ``index_select`` on the precomputed dense matrix, where it has at most --dense-limit elements (the
                          matrix the format exists to avoid; null otherwise)
              onehot      ``tn.tt_multiply`` on the one-hot batch [P, rows], at the smallest P only and where that operand has
                          at most --onehot-limit elements (null otherwise)
            ``dense_elements`` = rows cols, ``tt_parameters`` = the elements of the cores.

Every time is the best of --reps windows of calls between two HIP events on the current stream (the window ends in a
synchronise), after one warm-up call per shape and route; the routes alternate window by window; a window holds 20 calls at
P <= 2^12, 10 up to 2^16 and 3 above.  Without a GPU the tool stops: it never reports a CPU time as a device time.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT_TABLES = ["100,100,100:4,8,4:8", "100,100,100:4,8,4:16", "100,100,100:4,8,4:32", "16,16,16,16:4,4,4,4:16"]


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


def inner_for(P):
    return 20 if P <= 1 << 12 else 10 if P <= 1 << 16 else 3


def torch_step(Xg, G, idx, gather_limit):
    """Y[p] = Xg[p] @ G[:, idx[p]] for gathered rows Xg [P, D, R]: bmm with the gathered slices, in chunks of samples."""
    R, I, O, S = G.shape
    P = idx.shape[0]
    chunk = max(1, min(P, gather_limit // (R * O * S * G.element_size())))
    Gp = G.permute(1, 0, 2, 3).reshape(I, R, O * S)
    out = torch.empty((P, Xg.shape[1], O * S), dtype=G.dtype, device=G.device)
    for p0 in range(0, P, chunk):
        torch.bmm(Xg[p0:p0 + chunk], Gp[idx[p0:p0 + chunk]], out=out[p0:p0 + chunk])
    return out


def digits_of(rows, idims):
    cols, below = [], 1
    for n in idims:
        below *= n
    for n in idims:
        below //= n
        cols.append(torch.div(rows, below, rounding_mode="floor") % n)
    return cols


def torch_chain(cores, rows, idims, gather_limit):
    P = rows.shape[0]
    dg = digits_of(rows, idims)
    Z = cores[0][0][dg[0]]
    for k in range(1, len(cores)):
        Z = torch_step(Z, cores[k], dg[k], gather_limit).reshape(P, -1, cores[k].shape[3])
    return Z.reshape(P, -1)


def make_cores(idims, odims, rank, dtype, dev):
    d = len(idims)
    g = torch.Generator(device=dev).manual_seed(rank + 31 * d)
    rk = [1] + [rank] * (d - 1) + [1]
    return [torch.randn((rk[k], idims[k], odims[k], rk[k + 1]), generator=g, dtype=dtype, device=dev) / rk[k] ** 0.5 for k in range(d)]


def step_line(table, cores, idims, P, dtype, name, reps, gather_limit):
    from tntorch_amd import _hip

    dev = cores[0].device
    g = torch.Generator(device=dev).manual_seed(P)
    X, G = cores[0][0].contiguous(), cores[1]
    rows_x, D, R = X.shape
    _, I, O, S = G.shape
    table2 = torch.stack([torch.randint(0, rows_x, (P,), generator=g, device=dev), torch.randint(0, I, (P,), generator=g, device=dev)], dim=1)
    xrow, idx = table2[:, 0], table2[:, 1]
    Y = torch.empty((P, D, O, S), dtype=dtype, device=dev)
    ws = torch.empty(_hip.ttm_lookup_workspace_bytes(P, I), dtype=torch.uint8, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    es, inner = X.element_size(), inner_for(P)
    out = {"bench": "step", "table": table, "P": P, "D": D, "R": R, "I": I, "O": O, "S": S, "dtype": name, "reps": reps, "inner": inner,
           "flops": 2 * P * D * R * O * S, "bytes": (P * D * R + G.numel() + Y.numel()) * es}
    _hip.ttm_lookup_step(X, xrow, G, idx, flag, out=Y, workspace=ws)
    out["max_err_over_bound"] = None
    if P <= 1 << 16:   # (above, the comparison's own temporaries are several times the step's output)
        ref = torch_step(X[xrow], G, idx, gather_limit)
        mag = torch_step(X[xrow].abs(), G.abs(), idx, gather_limit)
        u = 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53
        out["max_err_over_bound"] = float(((Y.reshape(ref.shape) - ref).abs().double() / (2 * (R + 1) * u * mag.double())).max())
        del ref, mag
    assert int(flag.item()) == 0
    ms = alternate({"kernel": lambda: _hip.ttm_lookup_step(X, xrow, G, idx, flag, out=Y, workspace=ws),
                    "torch": lambda: torch_step(X[xrow], G, idx, gather_limit)}, reps, inner)
    for k in ("kernel", "torch"):
        out[k + "_ms"] = ms[k]
        out[k + "_tflops"] = out["flops"] / ms[k] * 1e-9
        out[k + "_tbs"] = out["bytes"] / ms[k] * 1e-9
    out["torch_over_kernel"] = ms["torch"] / ms["kernel"]
    return out


def lookup_line(table, ttm, cores, idims, odims, P, dtype, name, reps, gather_limit, dense, onehot_limit, smallest):
    import tntorch_amd as tn

    dev = cores[0].device
    nrows, ncols = 1, 1
    for a, b in zip(idims, odims):
        nrows, ncols = nrows * a, ncols * b
    g = torch.Generator(device=dev).manual_seed(P + 1)
    rows = torch.randint(0, nrows, (P,), generator=g, device=dev)
    inner = inner_for(P)
    out = {"bench": "lookup", "table": table, "idims": idims, "odims": odims, "rank": int(cores[0].shape[3]), "P": P, "dtype": name,
           "reps": reps, "inner": inner, "dense_elements": nrows * ncols, "tt_parameters": sum(c.numel() for c in cores)}
    y, yc = tn.tt_lookup(ttm, rows), torch_chain(cores, rows, idims, gather_limit)
    out["max_rel_diff_vs_chain"] = float((y - yc).abs().max() / yc.abs().max())
    del y, yc
    fns = {"tt_lookup": lambda: tn.tt_lookup(ttm, rows), "chain": lambda: torch_chain(cores, rows, idims, gather_limit)}
    if dense is not None:
        fns["dense"] = lambda: torch.index_select(dense, 0, rows)
    if smallest and P * nrows <= onehot_limit:
        hot = torch.zeros((P, nrows), dtype=dtype, device=dev)
        hot[torch.arange(P, device=dev), rows] = 1
        fns["onehot"] = lambda: tn.tt_multiply(ttm, hot)
    ms = alternate(fns, reps, inner)
    for k in ("tt_lookup", "chain", "dense", "onehot"):
        out[k + "_ms"] = ms.get(k)
    out["chain_over_tt_lookup"] = ms["chain"] / ms["tt_lookup"]
    out["dense_over_tt_lookup"] = ms["dense"] / ms["tt_lookup"] if "dense" in ms else None
    out["onehot_over_tt_lookup"] = ms["onehot"] / ms["tt_lookup"] if "onehot" in ms else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", nargs="+", default=DEFAULT_TABLES, help="i_1,..,i_d:o_1,..,o_d:rank")
    ap.add_argument("--samples", nargs="+", type=int, default=[1 << 12, 1 << 16, 1 << 20])
    ap.add_argument("--dtypes", nargs="+", default=["f32", "f64"], choices=["f32", "f64"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gather-limit", type=int, default=1 << 30, help="bytes of gathered slices per chunk of the torch routes")
    ap.add_argument("--dense-limit", type=int, default=1 << 28, help="largest dense matrix (elements) the dense comparator forms")
    ap.add_argument("--onehot-limit", type=int, default=1 << 31, help="largest one-hot operand (elements) of the tt_multiply comparator")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lookup_bench needs a GPU")
    import tntorch_amd as tn

    sink = open(a.out, "a") if a.out else None

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if sink:
            sink.write(text + "\n")
            sink.flush()

    dev = torch.device("cuda:0")
    for name in a.dtypes:
        dtype = torch.float32 if name == "f32" else torch.float64
        for table in a.tables:
            idims, odims, rank = table.split(":")
            idims, odims, rank = [int(v) for v in idims.split(",")], [int(v) for v in odims.split(",")], int(rank)
            cores = make_cores(idims, odims, rank, dtype, dev)
            ttm = tn.TTMatrix(cores, None, idims, odims)
            elements = 1
            for n in idims + odims:
                elements *= n
            dense = ttm.torch().contiguous() if elements <= a.dense_limit else None
            for P in a.samples:
                emit(step_line(table, cores, idims, P, dtype, name, a.reps, a.gather_limit))
                emit(lookup_line(table, ttm, cores, idims, odims, P, dtype, name, a.reps, a.gather_limit, dense, a.onehot_limit,
                                 P == min(a.samples)))
            del dense
    if sink:
        sink.close()


if __name__ == "__main__":
    main()

"""The backward of the TT-matrix product on one MI355X: the two fused kernels of one step (ttr_ttm_grad_input, ttr_ttm_grad_core)
next to the same products as batched ``ttr_gemm`` calls and next to torch autograd's backward of the step's einsum, and a whole
forward + backward of ``tn.tt_multiply`` next to torch autograd through the reference's chain written with torch ops.

    python tools/ttmatrix_grad_bench.py --out profiles/ttmatrix_grad_bench_mi355x.jsonl
    python tools/ttmatrix_grad_bench.py --step-layers 4,8,8,4:16:4096 --layers 4,8,8,4:16:256 --dtypes f32     # one corner

A layer is ``i_0,..,i_{d-1}:rank:batch`` as in tools/ttmatrix_bench.py (whose window helper, step shapes and torch chain are used
here).  Two kinds of JSON lines, each for fp32 and fp64:

  "grad_step"      the first, a middle and the last step of a layer: X [I, D, R], G [R, I, O, S], dY [D, O, S] random.  ms per call,
                   for ``input`` (dX from dY and G) and ``core`` (dG from X and dY):
                     kernel     ``_hip.ttm_grad_input`` / ``_hip.ttm_grad_core`` into preallocated outputs (core: + the slab sum
                                where D is cut; its workspace preallocated)
                     gemm       the same product as ONE batched ``ttr_gemm`` call over i: dX[i] = dY G[:, i]^T (batch stride 0 on
                                dY), dG[:, i] = X[i]^T dY written in place with ldc = I O S (split-K by the library's own rule,
                                workspace preallocated)
                     autograd   ``torch.autograd.grad`` of ``torch.einsum("idr,riob->dob", X, G)`` with respect to X resp. G
                   ``flops`` = 2 D (I R) (O S) for either product; ``input_bytes`` / ``core_bytes`` = the elements of the product's
                   three arrays once, in the dtype; ``*_tflops`` / ``*_tbs`` = those over the time: achieved rates of what the
                   algorithm needs, not counters.  ``*_max_err_over_bound``: the kernel against torch's result in units of the
                   step bounds 2 (O S + 1) u |dY| . |G| and 2 (D + 1) u |X|^T . |dY|.
  "grad_multiply"  forward + backward of a whole product of a batch [b, rows], gradients of every core and of x: ms per call
                     tn         ``tn.tt_multiply`` and ``torch.autograd.grad`` (d + d + d launches and two transposed copies)
                     torch      the reference's chain with torch ops (tools/ttmatrix_bench.tt_chain) and ``torch.autograd.grad``

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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ttmatrix_bench import DEFAULT_LAYERS, alternate, step_shapes, tt_chain  # noqa: E402

# the layers of the step table of DESIGN section 24
STEP_LAYERS = ["4,8,8,4:8:4096", "4,8,8,4:16:4096", "4,8,8,4:32:4096", "8,8,8,8:16:1024", "16,16,16,16:8:64"]


def gemm_routes(X, G, dY, dX, dG):
    """(grad_input, grad_core) as one batched ttr_gemm call each, writing where the kernels write."""
    from tntorch_amd import _hip

    I, D, R = X.shape
    N = G.shape[2] * G.shape[3]
    dt = _hip.dtype_code(X.dtype)
    L = _hip.lib()
    ws_in = _hip._workspace(L.ttr_gemm_workspace_bytes(dt, D, R, N, I), X.device)
    ws_core = _hip._workspace(L.ttr_gemm_workspace_bytes(dt, R, N, D, I), X.device)
    none = (None, 0, _hip.SCALE_NONE)

    def grad_input():    # dX[i] [D, R] = dY [D, N] (G[:, i] [R, N], rows I N apart)^T
        _hip._call("ttr_gemm", dt, 0, 1, D, R, N, dY.data_ptr(), N, 0, G.data_ptr(), I * N, N, dX.data_ptr(), R, D * R, *none, *none, I,
                   _hip._ptr(ws_in), int(ws_in.numel()) if ws_in is not None else 0)

    def grad_core():     # dG[:, i] [R, N], rows I N apart = X[i]^T [R, D] dY [D, N]
        _hip._call("ttr_gemm", dt, 1, 0, R, N, D, X.data_ptr(), R, D * R, dY.data_ptr(), N, 0, dG.data_ptr(), I * N, N, *none, *none, I,
                   _hip._ptr(ws_core), int(ws_core.numel()) if ws_core is not None else 0)

    return grad_input, grad_core


def step_line(layer, which, I, D, R, O, S, dtype, name, reps, inner):
    from tntorch_amd import _hip

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(I + 7 * R + 13 * S)
    X = torch.randn((I, D, R), generator=g, dtype=dtype, device=dev)
    G = torch.randn((R, I, O, S), generator=g, dtype=dtype, device=dev)
    dY = torch.randn((D, O, S), generator=g, dtype=dtype, device=dev)
    dX, dG = torch.empty_like(X), torch.empty_like(G)
    es = X.element_size()
    slab = _hip.ttm_grad_core_slab_rows(dtype, I, D, R, O, S)
    ws = _hip._workspace(_hip.ttm_grad_core_workspace_bytes(dtype, I, D, R, O, S), dev)
    out = {"bench": "grad_step", "layer": layer, "step": which, "I": I, "D": D, "R": R, "O": O, "S": S, "dtype": name, "reps": reps,
           "inner": inner, "flops": 2 * D * I * R * O * S, "input_bytes": (dY.numel() + G.numel() + dX.numel()) * es,
           "core_bytes": (X.numel() + dY.numel() + dG.numel()) * es, "slab_rows": slab, "slabs": -(-D // slab)}
    Xg, Gg = X.clone().requires_grad_(), G.clone().requires_grad_()
    Y = torch.einsum("idr,riob->dob", Xg, Gg)
    u = 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53
    _hip.ttm_grad_input(dY, G, out=dX)
    _hip.ttm_grad_core(X, dY, out=dG, workspace=ws)
    ref_x, ref_g = torch.autograd.grad(Y, [Xg, Gg], dY, retain_graph=True)
    mag = torch.einsum("dos,rios->idr", dY.abs(), G.abs())
    out["input_max_err_over_bound"] = float(((dX - ref_x).abs().double() / (2 * (O * S + 1) * u * mag.double())).max())
    mag = torch.einsum("idr,dos->rios", X.abs(), dY.abs())
    out["core_max_err_over_bound"] = float(((dG - ref_g).abs().double() / (2 * (D + 1) * u * mag.double())).max())
    gemm_input, gemm_core = gemm_routes(X, G, dY, torch.empty_like(X), torch.empty_like(G))
    cx, cg = torch.empty_like(X), torch.empty_like(G)
    check_input, check_core = gemm_routes(X, G, dY, cx, cg)
    fns = {"input_kernel": lambda: _hip.ttm_grad_input(dY, G, out=dX),
           "input_autograd": lambda: torch.autograd.grad(Y, [Xg], dY, retain_graph=True),
           "core_kernel": lambda: _hip.ttm_grad_core(X, dY, out=dG, workspace=ws),
           "core_autograd": lambda: torch.autograd.grad(Y, [Gg], dY, retain_graph=True)}
    # (a shape ttr_gemm refuses is reported as such, with null times, not hidden)
    for side, check, timed, got, ref in (("input", check_input, gemm_input, cx, ref_x), ("core", check_core, gemm_core, cg, ref_g)):
        try:
            check()
            out["gemm_" + side + "_max_rel_diff"] = float((got - ref).abs().max() / ref.abs().max())
            fns[side + "_gemm"] = timed
        except (ValueError, NotImplementedError, RuntimeError) as e:
            out["gemm_" + side + "_refused"] = str(e)
    del ref_x, ref_g, mag, cx, cg
    ms = alternate(fns, reps, inner)
    for side in ("input", "core"):
        for route in ("kernel", "gemm", "autograd"):
            k = side + "_" + route
            t = ms.get(k)
            out[k + "_ms"] = t
            out[k + "_tflops"] = out["flops"] / t * 1e-9 if t else None
            out[k + "_tbs"] = out[side + "_bytes"] / t * 1e-9 if t else None
            if route != "kernel":
                out[k + "_over_kernel"] = t / ms[side + "_kernel"] if t else None
    return out


def multiply_line(layer, dims, rank, batch, dtype, name, reps, inner):
    import tntorch_amd as tn

    dev = torch.device("cuda:0")
    d = len(dims)
    g = torch.Generator(device=dev).manual_seed(rank + batch)
    rk = [1] + [rank] * (d - 1) + [1]
    scale = [1.0 / (dims[k] * rk[k]) ** 0.5 for k in range(d)]       # keeps the product's entries of order 1
    tt = [(torch.randn((rk[k], dims[k], dims[k], rk[k + 1]), generator=g, dtype=dtype, device=dev) * scale[k]).requires_grad_()
          for k in range(d)]
    ttm = tn.TTMatrix(tt, None, dims, dims)
    rows = 1
    for n in dims:
        rows *= n
    x = torch.randn((batch, rows), generator=g, dtype=dtype, device=dev).requires_grad_()
    w = torch.randn((batch, rows), generator=g, dtype=dtype, device=dev)
    out = {"bench": "grad_multiply", "layer": layer, "dims": dims, "rank": rank, "batch": batch, "dtype": name, "reps": reps, "inner": inner}
    leaves = tt + [x]

    def ours():
        return torch.autograd.grad(tn.tt_multiply(ttm, x), leaves, w)

    def chain():
        return torch.autograd.grad(tt_chain(tt, x), leaves, w)

    a, b = ours(), chain()
    out["max_rel_diff"] = max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(a, b))
    del a, b
    ms = alternate({"tn": ours, "torch": chain}, reps, inner)
    out["tn_ms"], out["torch_ms"] = ms["tn"], ms["torch"]
    out["torch_over_tn"] = ms["torch"] / ms["tn"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step-layers", nargs="*", default=STEP_LAYERS, help="layers whose first / middle / last steps are timed")
    ap.add_argument("--layers", nargs="*", default=DEFAULT_LAYERS, help="layers whose whole forward + backward is timed")
    ap.add_argument("--dtypes", nargs="+", default=["f32", "f64"], choices=["f32", "f64"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ttmatrix_grad_bench needs a GPU")
    sink = open(a.out, "a") if a.out else None

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if sink:
            sink.write(text + "\n")
            sink.flush()

    def parse(layer):
        dims, rank, batch = layer.split(":")
        return [int(v) for v in dims.split(",")], int(rank), int(batch)

    for name in a.dtypes:
        dtype = torch.float32 if name == "f32" else torch.float64
        for layer in a.step_layers:
            for which, I, D, R, O, S in step_shapes(*parse(layer)):
                emit(step_line(layer, which, I, D, R, O, S, dtype, name, a.reps, a.inner))
        for layer in a.layers:
            emit(multiply_line(layer, *parse(layer), dtype, name, a.reps, a.inner))
    if sink:
        sink.close()


if __name__ == "__main__":
    main()

"""The trainable TT embedding (``tn.tt_embedding`` / ``tn.tt_embedding_bag``) on one MI355X: each kernel of the
backward, the segment sum, the torch ops of the backward and a whole training step, each next to (a) the route over the kernels
the library had before and (b) torch autograd / torch ops on the same GPU.

    python tools/embedding_bench.py --out profiles/embedding_bench_mi355x.jsonl
    python tools/embedding_bench.py --tables 16,16,16,16:4,4,4,4:16 --samples 4096 --dtypes f32          # one corner

A table is ``i_1,..,i_d:o_1,..,o_d:rank`` (every inner TT rank = rank).  The rows are drawn uniformly; ``"skew": true`` marks the
one batch per table and dtype (at the middle P of --samples) in which half the rows are row 0, so that one slice of every core
and one group of the first digit hold half the samples.  JSON lines, for fp32 and fp64, every P of --samples and every bag
length of --bags where it applies; every ``*_ms`` is ms per call, null where a route does not exist or was not run:

  "grad_core"    one per step k = 1 .. d - 1 (k counts the cores from 0): dG_k from Z_{k-1} and a random dY
                   kernel     ``_hip.ttm_lookup_grad_core`` into a preallocated dG with a preallocated workspace and the sorted
                              sample ids at hand (validation, histogram, scan, the GEMM launch, the sum of the partials)
                   existing   ``ttr_gather_grad`` on the P D expanded rows with the expanded permutation and a host-built plan
                              (built before the clock starts: its readback of the counts is NOT in the time), where O S <= 512;
                              for k = 1 the gathered copy of the first core's rows is in the time
                   torch      einsum + ``index_add_`` (``_hostops.ttm_lookup_grad_core``), in chunks of samples whose outer products
                              stay below --gather-limit bytes
                 ``flops`` = 2 P D R O S; ``slab_rows``, ``max_slabs`` of the slab rule
  "grad_input"   one per step: dZ_{k-1} from dY and G_k
                   kernel     ``_hip.ttm_lookup_grad_input`` (preallocated)
                   existing   ``ttr_ttm_lookup_step`` on dY with the core viewed [O S, I, R, 1] (a permuted view, read in place)
                   torch      ``bmm`` with the gathered slices, chunked as above
  "segment_sum"  the pooling of Y [P, cols] into bags of ``bag`` rows (``kind": "bags"``) and the sum of dZ_1 [P, O_1 r_1] over
                 the groups of the first digit through the sorted ids (``"kind": "first_digit"``)
                   kernel     ``_hip.segment_sum``
                   torch      ``index_add_`` (``_hostops.segment_sum``)
                 there is no earlier kernel for it (``existing_ms`` null); ``longest`` = the longest segment, which sits on
                 ceil(C / block) workgroups: the skewed first-digit line is what that costs
  "torch_ops"    the torch ops of the backward: ``sort_ms`` one stable ``torch.sort`` of a digit column, ``bag_ms`` the
                 ``searchsorted`` + ``index_select`` + weight of dY [P, cols] from dOut [P / bag, cols]
  "train"        forward + backward of ``tn.tt_embedding_bag`` (sum, no weights) with every core requiring grad
                   package    the call and ``backward``
                   existing   ``tn.tt_multiply`` on the one-hot batch and ``backward``: the only trainable device route before;
                              at the smallest P only and where the one-hot operand has at most --onehot-limit elements
                   torch      autograd through the host chain's ops (``_hostops.tt_lookup_chain`` + ``segment_sum``) on the GPU,
                              for P <= --autograd-limit (its saved slices are P R O S elements per core)
                 ``max_rel_diff_vs_torch``: the package's core gradients against that route's, relative to the largest entry

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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lookup_bench import DEFAULT_TABLES, alternate, inner_for, make_cores, torch_step  # noqa: E402


def torch_grad_core(Xg, dY, idx, I, limit):
    from tntorch_amd import _hostops

    P, D, R = Xg.shape
    chunk = max(1, min(P, limit // (R * dY.shape[2] * dY.shape[3] * Xg.element_size())))
    dG = None
    for p0 in range(0, P, chunk):
        part = _hostops.ttm_lookup_grad_core(Xg[p0:p0 + chunk], None, dY[p0:p0 + chunk], idx[p0:p0 + chunk], I)
        dG = part if dG is None else dG.add_(part)
    return dG


def draw_rows(nrows, P, skew, dev):
    g = torch.Generator(device=dev).manual_seed(P + (7 if skew else 1))
    rows = torch.randint(0, nrows, (P,), generator=g, device=dev)
    if skew:
        rows[torch.randperm(P, generator=g, device=dev)[:P // 2]] = 0
    return rows


def step_lines(head, cores, digits, kept, a):
    """The "grad_core" and "grad_input" lines of every step, and the first-digit "segment_sum" line."""
    from tntorch_amd import _hip, _hipops

    dev, dtype = cores[0].device, cores[0].dtype
    P, d = digits.shape[0], len(cores)
    inner, es = inner_for(P), cores[0].element_size()
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    g = torch.Generator(device=dev).manual_seed(3)
    for k in range(1, d):
        G = cores[k].contiguous()
        R, I, O, S = G.shape
        col = digits[:, k]
        perm = torch.sort(col, stable=True).indices
        X, xrow = (cores[0][0].contiguous(), digits[:, 0]) if k == 1 else (kept[k], None)
        D = X.shape[1]
        dY = torch.randn((P, D, O, S), generator=g, dtype=dtype, device=dev)
        dG = torch.empty((R, I, O, S), dtype=dtype, device=dev)
        ws = torch.empty(_hip.ttm_lookup_grad_core_workspace_bytes(dtype, P, D, R, I, O, S), dtype=torch.uint8, device=dev)
        slab = _hip.ttm_lookup_grad_core_slab_rows(dtype, P, D, R, I, O, S)
        fns = {"kernel": lambda: _hip.ttm_lookup_grad_core(X, xrow, dY, col, perm, flag, dG, workspace=ws),
               "torch": lambda: torch_grad_core(X[xrow] if xrow is not None else X, dY, col, I, a.gather_limit)}
        if O * S <= 512:
            rows_perm = (perm[:, None] * D + torch.arange(D, device=dev)[None, :]).reshape(-1)
            plan = _hipops.GradPlan((torch.bincount(col, minlength=I) * D).cpu().tolist(), dev)
            fns["existing"] = lambda: _hipops.gather_grad((X[xrow] if xrow is not None else X).reshape(P * D, R), dY.view(P * D, O * S),
                                                          rows_perm, plan)
            try:
                fns["existing"]()
            except NotImplementedError:   # (ranks outside ttr_gather_grad's envelope)
                del fns["existing"]
        ms = alternate(fns, a.reps, inner)
        yield dict(head, bench="grad_core", step=k, D=D, R=R, I=I, O=O, S=S, inner=inner, flops=2 * P * D * R * O * S, slab_rows=slab,
                   max_slabs=-(-P * D // slab) + I, kernel_ms=ms["kernel"], existing_ms=ms.get("existing"), torch_ms=ms["torch"],
                   kernel_tflops=2 * P * D * R * O * S / ms["kernel"] * 1e-9,
                   kernel_tbs=(P * D * (R + O * S) + G.numel()) * es / ms["kernel"] * 1e-9)
        dX = torch.empty((P, D, R), dtype=dtype, device=dev)
        ws_in = torch.empty(_hip.ttm_lookup_grad_input_workspace_bytes(P, I), dtype=torch.uint8, device=dev)
        ws_fw = torch.empty(_hip.ttm_lookup_workspace_bytes(P, I), dtype=torch.uint8, device=dev)
        Gt = G.reshape(R, I, O * S).permute(2, 1, 0)[..., None]                     # [O S, I, R, 1], read where it lies
        dYf = dY.view(P, D, O * S)
        fns = {"kernel": lambda: _hip.ttm_lookup_grad_input(dY, G, col, perm, flag, out=dX, workspace=ws_in),
               "existing": lambda: _hip.ttm_lookup_step(dYf, None, Gt, col, flag, out=dX, workspace=ws_fw),
               "torch": lambda: torch_step(dYf, Gt, col, a.gather_limit)}
        ms = alternate(fns, a.reps, inner)
        yield dict(head, bench="grad_input", step=k, D=D, R=R, I=I, O=O, S=S, inner=inner, flops=2 * P * D * R * O * S,
                   kernel_ms=ms["kernel"], existing_ms=ms["existing"], torch_ms=ms["torch"],
                   kernel_tflops=2 * P * D * R * O * S / ms["kernel"] * 1e-9,
                   kernel_tbs=(P * D * (R + O * S) + G.numel()) * es / ms["kernel"] * 1e-9)
        del dY, dG, dX, ws
    yield segment_line(dict(head, kind="first_digit"), digits[:, 0], cores[0].shape[1], cores[0].shape[2] * cores[0].shape[3], dtype, a)
    assert int(flag.item()) == 0


def segment_line(head, col, groups, C, dtype, a, bag=None):
    """``bag``: Y [P, C] into bags of that many rows; else the groups of the index column ``col`` through its sorted ids."""
    from tntorch_amd import _hip, _hostops

    dev, P = col.device, col.shape[0]
    Y = torch.randn((P, C), generator=torch.Generator(device=dev).manual_seed(5), dtype=dtype, device=dev)
    if bag is not None:
        perm, seg = None, torch.arange(P // bag + 1, device=dev) * bag
    else:
        srt = torch.sort(col, stable=True)
        perm, seg = srt.indices, torch.searchsorted(srt.values, torch.arange(groups + 1, device=dev))
    out = torch.empty((seg.shape[0] - 1, C), dtype=dtype, device=dev)
    ms = alternate({"kernel": lambda: _hip.segment_sum(Y, seg, perm=perm, out=out),
                    "torch": lambda: _hostops.segment_sum(Y, seg, None, perm)}, a.reps, inner_for(P))
    return dict(head, bench="segment_sum", segments=int(seg.shape[0] - 1), C=C, longest=int((seg[1:] - seg[:-1]).max().item()),
                bag=bag, kernel_ms=ms["kernel"], existing_ms=None, torch_ms=ms["torch"],
                kernel_tbs=(P + seg.shape[0] - 1) * C * Y.element_size() / ms["kernel"] * 1e-9)


def torch_ops_line(head, digits, ncols, bag, dtype, a):
    dev, P = digits.device, digits.shape[0]
    B = P // bag
    seg = torch.arange(B + 1, device=dev) * bag
    dOut = torch.randn((B, ncols), generator=torch.Generator(device=dev).manual_seed(6), dtype=dtype, device=dev)
    w = torch.ones(P, dtype=dtype, device=dev)
    col = digits[:, -1]

    def bag_ops():
        owner = torch.searchsorted(seg[1:].contiguous(), torch.arange(P, device=dev), right=True)
        return dOut.index_select(0, owner) * w[:, None]

    ms = alternate({"sort": lambda: torch.sort(col, stable=True).indices, "bag": bag_ops}, a.reps, inner_for(P))
    return dict(head, bench="torch_ops", bag=bag, sort_ms=ms["sort"], bag_ms=ms["bag"])


def train_line(head, cores, idims, odims, rows, bag, a, smallest):
    import tntorch_amd as tn
    from tntorch_amd import _hostops

    dev, dtype = cores[0].device, cores[0].dtype
    P = rows.shape[0]
    nrows = 1
    for n in idims:
        nrows *= n
    rows2d = rows.view(P // bag, bag)
    seg = torch.arange(P // bag + 1, device=dev) * bag
    leaves = [c.clone().requires_grad_(True) for c in cores]
    ttm = tn.TTMatrix(leaves, None, idims, odims)
    ncols = 1
    for n in odims:
        ncols *= n
    gout = torch.randn((P // bag, ncols), generator=torch.Generator(device=dev).manual_seed(9), dtype=dtype, device=dev)

    def package():
        for c in leaves:
            c.grad = None
        tn.tt_embedding_bag(ttm, rows2d).backward(gout)

    def autograd():
        for c in leaves:
            c.grad = None
        _hostops.segment_sum(_hostops.tt_lookup_chain(leaves, rows), seg).backward(gout)

    fns = {"package": package}
    if P <= a.autograd_limit:
        fns["torch"] = autograd
    if smallest and P * nrows <= a.onehot_limit:
        hot = torch.zeros((P, nrows), dtype=dtype, device=dev)
        hot[torch.arange(P, device=dev), rows] = 1

        def onehot():
            for c in leaves:
                c.grad = None
            tn.tt_multiply(ttm, hot).view(P // bag, bag, -1).sum(dim=1).backward(gout)

        fns["existing"] = onehot
    diff = None
    if "torch" in fns:
        package()
        ours = [c.grad.clone() for c in leaves]
        autograd()
        diff = max(float((o - c.grad).abs().max() / c.grad.abs().max()) for o, c in zip(ours, leaves))
    ms = alternate(fns, a.reps, inner_for(P))
    return dict(head, bench="train", bag=bag, package_ms=ms["package"], existing_ms=ms.get("existing"), torch_ms=ms.get("torch"),
                max_rel_diff_vs_torch=diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", nargs="+", default=DEFAULT_TABLES, help="i_1,..,i_d:o_1,..,o_d:rank")
    ap.add_argument("--samples", nargs="+", type=int, default=[1 << 12, 1 << 16, 1 << 20])
    ap.add_argument("--bags", nargs="+", type=int, default=[1, 32])
    ap.add_argument("--dtypes", nargs="+", default=["f32", "f64"], choices=["f32", "f64"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gather-limit", type=int, default=1 << 30, help="bytes of gathered slices / outer products per chunk of the torch routes")
    ap.add_argument("--autograd-limit", type=int, default=1 << 16, help="largest P of the torch autograd route of the train lines")
    ap.add_argument("--onehot-limit", type=int, default=1 << 31, help="largest one-hot operand (elements) of the tt_multiply route")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("embedding_bench needs a GPU")
    from tntorch_amd import _hipops, _hostops

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
            nrows, ncols = 1, 1
            for i, o in zip(idims, odims):
                nrows, ncols = nrows * i, ncols * o
            middle = sorted(a.samples)[len(a.samples) // 2]
            for P, skew in [(P, False) for P in a.samples] + [(middle, True)]:
                head = {"table": table, "rank": rank, "P": P, "dtype": name, "skew": skew, "reps": a.reps}
                rows = draw_rows(nrows, P, skew, dev)
                digits = _hostops.lookup_digits(cores, rows)
                _, flag, kept = _hipops.tt_lookup_steps(cores, digits, keep=[True] * len(cores))
                assert int(flag.item()) == 0
                for line in step_lines(head, cores, digits, kept, a):
                    emit(line)
                del kept
                for bag in a.bags:
                    emit(segment_line(dict(head, kind="bags"), digits[:, 0], None, ncols, dtype, a, bag=bag))
                    emit(torch_ops_line(head, digits, ncols, bag, dtype, a))
                    emit(train_line(head, cores, idims, odims, rows, bag, a, P == min(a.samples) and not skew))
    if sink:
        sink.close()


if __name__ == "__main__":
    main()

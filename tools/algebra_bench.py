"""``tn.tt_apply`` and its kernel ``ttr_core_compose`` on one MI355X, next to the same cores built by ``torch.einsum`` on the
device and, where the dense vector fits, to ``tn.tt_multiply`` on ``t.torch()``.  Reads nothing but this package.

    python tools/algebra_bench.py                    # every row
    python tools/algebra_bench.py --only step --reps 20
    python tools/algebra_bench.py --only whole

One-step rows (``kind: step``): one core, A [r, P, J, r] and B [s, J, Q, s] with r = s in {8, 16, 32} and J in {4, 16, 64}, for
the three products -- ``apply`` (P = 1, Q = 16: a core of vec(t) @ M), ``apply_t`` (P = 16, Q = 1: M @ vec(u)) and ``matmul``
(P = Q = 8) -- in fp32 and fp64, cores ``randn``:
  core_compose   ``_hip.core_compose`` (one launch; the allocation of the output included)
  einsum         ``torch.einsum("rpjs,ajqb->rapqsb", A, B).reshape(...)``, the same core on the same GPU
Each variant is warmed up, the two alternate inside the repetition loop, a timed window is ``inner`` calls back to back between
device events (``inner`` grows until a window writes at least 4 GiB, at most 200), and the figure is the median over --reps of
the window / inner.  A row reports the bytes of the output, E w, over that time in TB/s and as a fraction of the 8 TB/s peak --
the kernel's lower bound for J up to a few dozen (2 J E flops against E w bytes); for the small cores the figure is a measure of
the launch, not of the memory system, and says so through ``output_bytes``.  ``ratio_einsum_over_kernel`` >= 1: the kernel is
not slower.  The largest difference between the two cores relative to the largest entry is recorded.

Whole-call rows (``kind: whole``): ``tn.tt_apply(M, t, rmax=r)`` with matrix rank 8 and train rank r = 16 on a [16]^4 x [16]^4
operator and on an 8-mode [8]^8 x [8]^8 operator, fp32 and fp64 (median of --reps, the variants alternating):
  tt_apply        as a user calls it: d launches of ttr_core_compose and one round_tt
  einsum_round    the same cores from the einsum above, then the same round_tt
  compose_only    the d launches alone;  round_only: round_tt on a fresh copy of the exact train
  tt_multiply     ``tn.tt_multiply(M, t.torch().reshape(1, -1))`` where the dense vector has at most 2^26 entries: the route
                  through the dense vector (decompression included), whose result is dense, not a train
One JSON line per row, appended to profiles/algebra_bench_mi355x.jsonl.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "algebra_bench_mi355x.jsonl")
HBM_PEAK = 8.0e12
WINDOW_BYTES = 4 << 30


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


def einsum_core(A, B):
    R1, P, _, R2 = A.shape
    S1, _, Q, S2 = B.shape
    return torch.einsum("rpjs,ajqb->rapqsb", A, B).reshape(R1 * S1, P, Q, R2 * S2)


def repeated(fn, inner):
    def f():
        for _ in range(inner):
            out = fn()
        return out
    return f


def emit(line):
    print(json.dumps(line), flush=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(line) + "\n")


def step_rows(args, dev):
    from tntorch_amd import _hip

    products = {"apply": (1, 16), "apply_t": (16, 1), "matmul": (8, 8)}
    for dt in (torch.float32, torch.float64):
        for name, (P, Q) in products.items():
            for r in (8, 16, 32):
                for J in (4, 16, 64):
                    g = torch.Generator().manual_seed(r * 100 + J)
                    A = torch.randn((r, P, J, r), dtype=torch.float64, generator=g).to(dt).to(dev)
                    B = torch.randn((r, J, Q, r), dtype=torch.float64, generator=g).to(dt).to(dev)
                    E = r * r * P * Q * r * r
                    nbytes = E * A.element_size()
                    inner = max(1, min(200, -(-WINDOW_BYTES // nbytes)))
                    fns = {"core_compose": repeated(lambda: _hip.core_compose(A, B), inner),
                           "einsum": repeated(lambda: einsum_core(A, B), inner)}
                    ms, last = alternate(fns, args.reps)
                    ms = {k: {q: v / inner for q, v in d.items()} for k, d in ms.items()}
                    diff = float((last["core_compose"] - last["einsum"]).abs().max()) / float(last["einsum"].abs().max())
                    rate = {k: nbytes / (ms[k]["median_ms"] * 1e-3) for k in ms}
                    emit({"kind": "step", "product": name, "dtype": str(dt), "shape": [r, P, J, r, r, Q, r], "output_elements": E,
                          "output_bytes": nbytes, "flops": 2 * J * E, "reps": args.reps, "inner": inner, "ms": ms,
                          "output_TB_per_s": {k: v / 1e12 for k, v in rate.items()},
                          "fraction_of_8TBs_peak": {k: v / HBM_PEAK for k, v in rate.items()},
                          "ratio_einsum_over_kernel": ms["einsum"]["median_ms"] / ms["core_compose"]["median_ms"],
                          "largest_difference_over_largest_entry": diff})


def whole_rows(args, dev):
    import tntorch_amd as tn
    from tntorch_amd import _hip

    operators = {"16^4": [16] * 4, "8^8": [8] * 8}
    rm, r = 8, 16
    for dt in (torch.float32, torch.float64):
        for name, dims in operators.items():
            d = len(dims)
            g = torch.Generator().manual_seed(d)
            rk, rt = [1] + [rm] * (d - 1) + [1], [1] + [r] * (d - 1) + [1]
            G = [(torch.randn((rk[k], n, n, rk[k + 1]), dtype=torch.float64, generator=g) / (n * rm ** 0.5)).to(dt).to(dev)
                 for k, n in enumerate(dims)]
            T = [(torch.randn((rt[k], n, rt[k + 1]), dtype=torch.float64, generator=g) / r ** 0.5).to(dt).to(dev) for k, n in enumerate(dims)]
            M, t = tn.TTMatrix(G, None, dims, dims), tn.Tensor(T)
            A = [c[:, None].contiguous() for c in T]

            def compose():
                return [_hip.core_compose(x, y)[:, 0] for x, y in zip(A, G)]

            def einsum_round():
                out = tn.Tensor([einsum_core(x, y)[:, 0] for x, y in zip(A, G)])
                out.round_tt(eps=0, rmax=r)
                return out

            exact = compose()

            def round_only():
                out = tn.Tensor([c.clone() for c in exact])
                out.round_tt(eps=0, rmax=r)
                return out

            fns = {"tt_apply": lambda: tn.tt_apply(M, t, rmax=r), "einsum_round": einsum_round, "compose_only": compose,
                   "round_only": round_only}
            numel = 1
            for n in dims:
                numel *= n
            if numel <= 1 << 26:
                fns["tt_multiply"] = lambda: tn.tt_multiply(M, t.torch().reshape(1, -1))
            ms, last = alternate(fns, args.reps)
            line = {"kind": "whole", "operator": name, "dtype": str(dt), "matrix_rank": rm, "train_rank": r, "rmax": r, "reps": args.reps,
                    "ms": ms, "ranks_exact": [1] + [int(c.shape[-1]) for c in exact], "ranks_result": last["tt_apply"].ranks_tt.tolist(),
                    "ratio_einsum_round_over_tt_apply": ms["einsum_round"]["median_ms"] / ms["tt_apply"]["median_ms"],
                    "compose_share_of_tt_apply": ms["compose_only"]["median_ms"] / ms["tt_apply"]["median_ms"]}
            if "tt_multiply" in ms:
                line["dense_vector_entries"] = numel
                line["ratio_tt_multiply_over_tt_apply"] = ms["tt_multiply"]["median_ms"] / ms["tt_apply"]["median_ms"]
                dense = last["tt_apply"].torch().reshape(-1)
                ref = last["tt_multiply"][0]
                line["relative_difference_to_tt_multiply"] = float((dense - ref).norm() / ref.norm())
            emit(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["step", "whole"], default=None)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("algebra_bench needs a GPU")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if args.only in (None, "step"):
        step_rows(args, dev)
    if args.only in (None, "whole"):
        whole_rows(args, dev)


if __name__ == "__main__":
    main()

"""Sparse TT-SVD from samples (tn.sparse_tt_svd) on the device: a work model of every step, time per call, and the reference's
dense formulation run through torch on the same device at a size where its D still fits.

    python tools/sparse_bench.py [--dtype fp32] [--shape 128 64 64 64] [--log2p 18] [--rmax 4] [--reps 5] [--dense-log2p 14]

Model of one step (n = r I rows, C columns, m_c blocks in column c):
  gram      sum_c m_c (m_c + 1) / 2 * r^2 multiply-adds (j >= i only), the block table (nb (r values + 3 int32)) read once per
            (a, b) tile and j range of a mode index's workgroups (`gram_table_bytes`), n^2 elements written per part and once
            more by the finishing kernel
  project   nb r q multiply-adds, the block table read once, C q elements written
The dense formulation costs n^2 C (D D^T) + n q C (left^T D) multiply-adds and n C elements of D.
Prints one JSON object per line: the per-step model with measured kernel times, then the totals.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tntorch_amd as tn  # noqa: E402
from tntorch_amd import _hip, _hipops, interpolation  # noqa: E402


def samples(shape, P, seed, device):
    g = torch.Generator().manual_seed(seed)
    flat = torch.randperm(int(np.prod(shape)), generator=g)[:P]
    X = torch.stack(torch.unravel_index(flat, shape), dim=1)
    return X.to(device), torch.randn(P, generator=g).to(device)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts))


def dense_reference(X, y, eps, shape, rmax):
    """The reference's formulation (dense D per step, D D^T, eigh, left^T D) in torch on y's device."""
    N = len(shape)
    delta = eps / (N - 1) ** 0.5 * float(torch.norm(y))
    cur = list(shape)
    for n in range(1, N):
        u, v = torch.unique(X[:, 1:], dim=0, return_inverse=True)
        D = torch.zeros(cur[0], len(u), dtype=y.dtype, device=y.device)
        D[X[:, 0], v] = y
        w, vec = torch.linalg.eigh(D @ D.t())
        w = torch.clamp(w, min=0).flip(0)
        tail = torch.cumsum(w.flip(0), 0)
        kept = len(w) - int((tail <= delta**2).sum())
        rank = max(1, min(rmax, kept, len(u)))
        FD = vec.flip(1)[:, :rank].t() @ D
        rows = torch.arange(rank, device=y.device)[None, :].expand(len(u), rank)
        X = torch.cat([rows.reshape(-1, 1), u[:, None, :].expand(-1, rank, -1).reshape(len(u) * rank, -1)], dim=1)
        y = FD.t().reshape(-1)
        if n < N - 1:
            X = torch.cat([X[:, 0:1] * cur[1] + X[:, 1:2], X[:, 2:]], dim=1)
            cur = [rank * cur[1]] + cur[2:]
    return y


def table_reads(r, I):
    """How often ttr_sparse_gram reads a block of the table: once per (a, b) tile and per j range at or above its mode index
    (half the j ranges on average) -- the tiling of csrc/ttr_sparse.hip (rank tiles of 32, 8 x 256 accumulators)."""
    ta = min(r, 32)
    nt = -(-r // ta)
    jt = max(1, min(I, 64, 2048 // (ta * ta)))
    nj = -(-I // jt)
    return nt * nt * (nj + 1) / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "fp64"])
    ap.add_argument("--shape", type=int, nargs="+", default=[128, 64, 64, 64])
    ap.add_argument("--log2p", type=int, default=18)
    ap.add_argument("--rmax", type=int, default=4)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dense-log2p", type=int, default=14, help="samples of the dense comparison (its D: n x ~P elements)")
    a = ap.parse_args()
    dtype = torch.float32 if a.dtype == "fp32" else torch.float64
    es = 4 if a.dtype == "fp32" else 8
    X, y = samples(a.shape, 1 << a.log2p, 0, "cuda")
    y = y.to(dtype)

    steps = []
    orig = _hipops.sparse_step

    def spy(V, I, colptr, blk_i, blkcol, delta2_dev, cap):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        left, W = orig(V, I, colptr, blk_i, blkcol, delta2_dev, cap)
        torch.cuda.synchronize()
        nb, r = V.shape
        m = (colptr[1:] - colptr[:-1]).double()
        q, C = W.shape[1], W.shape[0]
        steps.append({"r": r, "I": I, "n": r * I, "blocks": nb, "columns": C, "q": q, "max_m": int(m.max()),
                      "gram_fma": float((m * (m + 1) / 2).sum()) * r * r, "project_fma": float(nb) * r * q,
                      "dense_fma": float(r * I) ** 2 * C + float(r * I) * q * C, "dense_D_bytes": r * I * C * es,
                      "table_bytes": nb * (r * es + 12), "gram_table_bytes": nb * (r * es + 12) * table_reads(r, I),
                      "parts": _hip.sparse_gram_parts(dtype, r, I, nb),
                      "step_ms": 1e3 * (time.perf_counter() - t0)})
        return left, W

    _hipops.sparse_step = spy
    try:
        tn.sparse_tt_svd(X, y, a.eps, shape=a.shape, rmax=a.rmax)  # warm-up
        steps.clear()
        t = tn.sparse_tt_svd(X, y, a.eps, shape=a.shape, rmax=a.rmax)
    finally:
        _hipops.sparse_step = orig
    for k, s in enumerate(steps):
        print(json.dumps({"step": k + 1, **s}))
    med, best = timed(lambda: tn.sparse_tt_svd(X, y, a.eps, shape=a.shape, rmax=a.rmax), a.reps)
    out = {"what": "tn.sparse_tt_svd", "dtype": a.dtype, "shape": a.shape, "P": 1 << a.log2p, "rmax": a.rmax,
           "ranks": [int(r) for r in t.ranks_tt], "call_ms_median": 1e3 * med, "call_ms_min": 1e3 * best, "reps": a.reps}
    Xd, yd = samples(a.shape, 1 << a.dense_log2p, 0, "cuda")
    yd = yd.to(dtype)
    ms, mb = timed(lambda: tn.sparse_tt_svd(Xd, yd, a.eps, shape=a.shape, rmax=a.rmax), a.reps)
    ds, db = timed(lambda: dense_reference(Xd, yd, a.eps, a.shape, a.rmax), a.reps)
    out["compare_P"] = 1 << a.dense_log2p
    out["compare_sparse_ms_median"], out["compare_dense_torch_ms_median"] = 1e3 * ms, 1e3 * ds
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Record tests/golden/indexing_f64.npz from the unmodified reference (tntorch), as oracle/gen_golden.py does for rounding.

    python tools/gen_indexing_golden.py /path/to/tntorch-checkout

Covers every key of the reference's test_indexing.py (test_mixed, test_batch, test_slicing) on TT, TT-Tucker, boundary ranks
above 1 and batch trains.  Stored per case: the input cores / factors; per key: the return type (scalar or Tensor), the dense
value (``.torch()`` of a returned Tensor), the shapes of the returned cores and factors, and whether the result is a batch.
Keys are stored as JSON (slices, None, Ellipsis and index arrays encoded).  Only data is written; no reference code is copied.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "indexing_f64.npz")

MIXED = [
    ([0, 0, 0], None, None, 3), ([0, 0, 0, 0, 0], slice(None), None, 0), (0, [0]), ([0], [0]), ([0], None, None, None, 0, 1),
    (slice(None), [0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5]), ([0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5]),
    (slice(None), slice(None), slice(None), 0), (slice(None), slice(None), [0, 1], 0), (0, np.array([0]), None, 0),
    (slice(None), slice(None), slice(None), slice(None), None), (None, slice(None), slice(None), slice(None), slice(None), None),
    (None, slice(None), slice(None), slice(None), slice(None)),
    # beyond the reference's lists: all-int keys, negative ints, Ellipsis, steps, a [P, N] matrix
    (1, 2, 3, 4), (-1, 2, -3, 0), (Ellipsis, 2), slice(1, 5, 2), (slice(None), slice(None, None, 3), -1),
    np.array([[0, 1, 2, 3], [5, 5, 5, 4], [1, 1, 1, 1], [5, 0, 4, 0]]),
]
BATCH = [
    ([0, 0, 0], None, None, 3), ([0, 0, 0, 0, 0], slice(None), None, 0), (0, [0]), ([0], None, None, None, 0, 1),
    (slice(None), [0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5]), (slice(None), slice(None), slice(None), 0),
    (slice(None), slice(None), [0, 1], 0), (0, np.array([0]), None, 0), (slice(None), slice(None), slice(None), slice(None), None),
    0, [0, 1], (slice(None), 1, 2, 3), (1, slice(None), 2), (2, 1, 2, 3),
]
SLICING = [slice(None), (slice(None), slice(1, None)), (slice(None), slice(0, 2, None), slice(0, 1))]


def encode(k):
    if isinstance(k, tuple):
        return {"tuple": [encode(x) for x in k]}
    if isinstance(k, np.ndarray):
        return {"ndarray": k.tolist()}
    if isinstance(k, list):
        return {"list": [encode(x) for x in k]}
    if isinstance(k, slice):
        return {"slice": [k.start, k.stop, k.step]}
    if k is None:
        return {"none": True}
    if k is Ellipsis:
        return {"ellipsis": True}
    return int(k)


def main(ref_path):
    sys.path.insert(0, ref_path)
    import tntorch as tn

    torch.set_default_dtype(torch.float64)
    torch.manual_seed(0)
    cases = []
    t = tn.rand([6, 6, 6, 5], ranks_tt=3)
    cases.append(("tt", t, MIXED))
    cases.append(("tt_tucker", tn.rand([6, 6, 6, 5], ranks_tt=3, ranks_tucker=2), MIXED))
    t = tn.rand([6, 6, 6, 5], ranks_tt=3)
    t.cores[0] = torch.randn(2, 6, 3)
    t.cores[-1] = torch.randn(3, 5, 2)
    cases.append(("tt_boundary", t, MIXED))
    cases.append(("batch_tt", tn.rand([6, 6, 6, 5], ranks_tt=3, batch=True), BATCH))
    cases.append(("batch_tucker", tn.rand([6, 6, 6, 5], ranks_tucker=3, batch=True), BATCH))
    cases.append(("slicing", tn.rand([1, 3, 1, 2, 1], ranks_tt=3, ranks_tucker=2), SLICING))

    arrays, meta = {}, []
    for ci, (name, t, keys) in enumerate(cases):
        for n, c in enumerate(t.cores):
            arrays[f"c{ci}_core{n}"] = c.numpy()
            if t.Us[n] is not None:
                arrays[f"c{ci}_U{n}"] = t.Us[n].numpy()
        entries = []
        for ki, k in enumerate(keys):
            r = t[k]
            e = {"key": encode(k)}
            if isinstance(r, tn.Tensor):
                e["type"] = "tensor"
                e["batch"] = bool(r.batch)
                e["core_shapes"] = [list(c.shape) for c in r.cores]
                e["U_shapes"] = [None if U is None else list(U.shape) for U in r.Us]
                arrays[f"c{ci}_k{ki}"] = r.torch().numpy()
            else:
                e["type"] = "scalar"
                arrays[f"c{ci}_k{ki}"] = r.numpy()
            entries.append(e)
        meta.append({"name": name, "batch": bool(t.batch), "ncores": len(t.cores),
                     "tucker": [U is not None for U in t.Us], "keys": entries})
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}: {len(cases)} cases, {sum(len(m['keys']) for m in meta)} keys")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("TNTORCH_REF", "."))

"""Cycle stamps inside the top-r first pass (ttr_eigh_top; library built with -DTTR_EIGH_STAMPS:
    bash tools/build_variant.sh stamps ttr_eigh.hip -DTTR_EIGH_STAMPS;  TTR_LIB_PATH=tntorch_amd/libttround_stamps.so python tools/probes/eigh_top_stamps.py
One block of a launch: wave 0 (tridiagonalisation, eigenvalues, twisted factorisations) and wave 1 (Q formation, eigenvalues,
back-transformation + Newton-Schulz on the matrix cores), for a full 64 x 64 problem and for one that shrinks to 32 x 32 -- a lone
matrix, and blocks of the first and of a later round of a 4096-matrix launch in the unrolled and in the lean build of the 32-row
instance (TTR_KNOB_EIGH_SMALL = 1 / 2).  Printed per phase: cycles spent in it (differences of consecutive stamps)."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from tntorch_amd import _hip

L = _hip.lib()
L.ttr_debug_set_eigh_stamps.argtypes = [ctypes.c_void_p]
L.ttr_debug_set_eigh_stamps.restype = None
L.ttr_debug_set_eigh_stamp_block.argtypes = [ctypes.c_longlong]
L.ttr_debug_set_eigh_stamp_block.restype = None
W0 = ["tridiag", "(dup)", "multisection", "twisted fact.", "(dup)", "barrier B1", "vectors written", "barrier B2", "sigma + zero columns"]
W1 = ["Q formed (from block start)", "multisection", "twisted fact.", "barrier B1", "vectors written", "barrier B2", "Z^T Q^T", "S + Newton-Schulz", "stored"]


def run(B, kind, knob, block):
    torch.manual_seed(0)
    M = torch.randn(B, 64, 256, device="cuda")
    if kind != "full 64":
        M[:, 32:] = 0
    G = _hip.rowgram(M)
    buf = torch.zeros(64, dtype=torch.int64, device="cuda")
    _hip.set_knob(_hip.KNOB_EIGH_SMALL, knob)
    try:
        _hip.eigh_top(G, 32, 0.125)
        torch.cuda.synchronize()
        L.ttr_debug_set_eigh_stamp_block(block)
        L.ttr_debug_set_eigh_stamps(buf.data_ptr())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        V, sg, info, flat = _hip.eigh_top(G, 32, 0.125)
        e1.record()
        torch.cuda.synchronize()
    finally:
        L.ttr_debug_set_eigh_stamps(None)
        L.ttr_debug_set_eigh_stamp_block(0)
        _hip.set_knob(_hip.KNOB_EIGH_SMALL, 2)
    st = buf.cpu().tolist()
    w0 = [x for x in st[:31] if x]
    w1 = [x for x in st[32:] if x]
    print(f"B={B} {kind}, knob {knob}, block {block}: launch {e0.elapsed_time(e1) * 1e3:.0f} us, flat {int(flat[block])}, "
          f"load + scale {w0[0] - st[31]}, block total from there {max(w0[-1], w1[-1]) - w0[0]}")
    print("   wave 0:", ", ".join(f"{n} {b - a}" for n, a, b in zip(W0, w0, w0[1:])))
    print("   wave 1:", ", ".join(f"{n} {b - a}" for n, a, b in zip(W1, [w0[0]] + w1, w1)))


for kind in ("full 64", "zero tail (32)"):
    run(1, kind, 2, 0)
for knob in (1, 2):
    for block in (700, 2600):
        run(4096, "zero tail (32)", knob, block)

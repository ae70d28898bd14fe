"""The four-wave pair instance of qr_factor (TTR_KNOB_QR_PAIR4) against the 8-wave instance for four live row groups, on the
level-1 problem of the headline taken as a plain matrix (so that the launch is a level 0 and writes the cycle stamps): B matrices of
256 x 64, four stacked 64 x 64 R factors of numerical rank 32.  Prints per variant the launch time and, for blocks at different
places of the grid, total cycles and the deltas per panel [transpose + rank test, phases, T / W, update]; then the last-bit
difference in R between the four-wave pair instance and the single-step kernel on the first core of g + g ([G, G], 64 x 64).
    python tools/probes/qr_pair4_stamps.py [B]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from tntorch_amd import _hip as h

L = h.lib()
B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
torch.manual_seed(0)
leaf = lambda: torch.cat([torch.triu(torch.randn(B, 32, 64, device="cuda")),
                          1e-7 * torch.triu(torch.randn(B, 32, 64, device="cuda"), diagonal=32)], dim=1)
A = torch.cat([leaf() for _ in range(4)], dim=1).contiguous()
buf = torch.zeros(64, dtype=torch.int64, device="cuda")
res = {}
for tag, pair4, nw4 in (("8-wave, four live groups", 1, 4), ("4-wave pair", 3, 0)):
    h.set_knob(h.KNOB_QR_PAIR4, pair4); h.set_knob(h.KNOB_QR_F64_NW4, nw4)
    h.qr_factor(A); torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f = h.qr_factor(A); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    res[tag] = f.R.clone()
    print(f"---- {tag}: launch {min(ts):.1f} - {max(ts):.1f} us")
    for by in (0, B // 4, B // 2, 3 * B // 4, B - 3):
        h.set_knob(h.KNOB_QR_STAMP_BX, 0); h.set_knob(h.KNOB_QR_STAMP_BY, by)
        L.ttr_debug_set_qr_stamps(buf.data_ptr()); buf.zero_()
        h.qr_factor(A); torch.cuda.synchronize()
        L.ttr_debug_set_qr_stamps(None)
        st = [x for x in buf.cpu().tolist() if x != 0]
        d = [st[i + 1] - st[i] for i in range(len(st) - 1)]
        print(f"block (0, {by}): total {st[-1] - st[0]}  load + guard {d[0]}  panels {[d[1 + 4 * k: 5 + 4 * k] for k in range(4)]}")
h.set_knob(h.KNOB_QR_STAMP_BX, 0); h.set_knob(h.KNOB_QR_STAMP_BY, 0)
print("R equal:", torch.equal(*res.values()))

# the first core: pair steps with the rank-revealing early exit against the single-step kernel
G = torch.randn(B, 64, 32, device="cuda")
F = torch.cat([G, G], dim=2).contiguous()
out = {}
for tag, pair4 in (("single-step", 1), ("4-wave pair", 3)):
    h.set_knob(h.KNOB_QR_PAIR4, pair4); h.set_knob(h.KNOB_QR_F64_NW4, 0)
    h.qr_factor(F); torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f = h.qr_factor(F); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    out[tag] = f.R.double()
    print(f"first core, {tag}: launch {min(ts):.1f} - {max(ts):.1f} us")
h.set_knob(h.KNOB_QR_PAIR4, 1)
a, b = out.values()
print(f"first core, R: max |dR| / max |R| = {((a - b).abs().max() / a.abs().max()).item():.3e} over all rows; "
      f"rows 0 .. 31: {((a - b)[:, :32].abs().max() / a.abs().max()).item():.3e}; entries that differ: {(a != b).float().mean().item():.3f}")

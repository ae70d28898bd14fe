#!/usr/bin/env python3
"""Benchmark of the TT rounding hot path on MI355X.

Workload (BASELINE.json `metric`, SURVEY 8d "M"): round_tt(rmax=32) of 64^8 tensors held in TT
format with rank 64 (t = g+g, g = randn-core TT of rank 32, float32) -- a dense 64^8 tensor
(1.1 PB) cannot exist, so "64^8 -> rank 32" is a TT-to-TT rounding.  One "step" rounds a batch
of B = 4096 independent tensors resident in HBM (B per GPU; weak scaling over ranks) and, for N > 1,
gathers the rounded cores on rank 0 with a single RCCL gather.

    python bench.py --gpus 1 --steps 5 --warmup 2
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W
    python bench.py --gpus 1 --steps 5 --warmup 2 --full   # + roofline, parity, extras, configs, CPU baseline
    python bench.py --config c3        # BASELINE config C3 (512 dense 32^5 -> rank 8), one line in the same format
    python bench.py --config c1        # BASELINE config C1 class (dense 64^k -> rank 16, the largest k that fits)

A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the line: nothing else.  Everything that
takes runs of its own -- the per-kernel roofline pass, the parity check against the oracle, the small-batch / B = 2048 /
decaying-spectrum extras, BASELINE's other configs, the CPU baseline, the N > 1 gather-alone timing -- runs with --full.

Prints ONE JSON line on rank 0 (see DESIGN.md "Measurement" for the definition of every field).
"""
import argparse
import contextlib
import hashlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

N_CORES, MODE, R_IN, R_OUT = 8, 64, 64, 32
HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy)
MFMA_F32_PEAK_TF = 157.3    # MI355X_MICROARCH.md: fp32-input MFMA = the fp32 vector rate (no xf32 on gfx950)
RIDGE = MFMA_F32_PEAK_TF * 1e12 / (HBM_PEAK_GBS * 1e9)   # 19.7 flop/B
FLOP_PER_TENSOR = 8.72e8    # SURVEY 8d, algorithmic flops of one 64^8 r64->r32 rounding
BYTES_PER_TENSOR = 2.69e7   # SURVEY 8d, algorithmic bytes (every core read once / written once per sweep)
REFERENCE_FACTOR = 1.2      # the oracle (port) takes 48 ms per 64^8 train where the reference takes 39 ms ('eig', 8 threads, build container)


def make_input(B, device, seed):
    """t = g + g with g = tn.randn([64]*8, ranks_tt=32) per batch item, built on the device."""
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    r = [1] + [R_OUT] * (N_CORES - 1) + [1]
    cores = []
    for k in range(N_CORES):
        g = torch.randn((B, r[k], MODE, r[k + 1]), generator=gen, device=device, dtype=torch.float32)
        if k == 0:
            c = torch.cat([g, g], dim=-1)
        elif k == N_CORES - 1:
            c = torch.cat([g, g], dim=-3)
        else:
            z = torch.zeros_like(g)
            c = torch.cat([torch.cat([g, z], dim=-1), torch.cat([z, g], dim=-1)], dim=-3)
        cores.append(c.contiguous())
    return cores


def make_decaying_input(B, device, seed, decay):
    """SURVEY 8d's second input variant of the metric: the same shapes (64^8, rank 64, fp32), i.i.d. normal cores of unit column
    variance with rank index j of every bond scaled by 2^(-decay j) -- bond singular values ~ 2^(-decay j): the kept spectrum is
    NOT flat, so neither the one-pass shortcut nor the top-r first pass applies (tests/test_gpu_parity.py: `_decaying_tt`)."""
    import math

    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    r = [1] + [R_IN] * (N_CORES - 1) + [1]
    cores = []
    for k in range(N_CORES):
        c = torch.randn((B, r[k], MODE, r[k + 1]), generator=gen, device=device, dtype=torch.float32)
        c.mul_(1.0 / math.sqrt(r[k] * MODE))
        if k < N_CORES - 1:
            c.mul_(2.0 ** (-decay * torch.arange(r[k + 1], device=device, dtype=torch.float32)))
        cores.append(c)
    return cores


def decaying_parity(inp, out, item):
    """One item of a decaying-spectrum batch against the oracle run in float64 on the same fp32 cores (the bounds of
    tests/test_gpu_parity.py::test_decaying_spectrum_metric_shape): identical ranks, bond singular values to 4e-6 sigma_max,
    right-orthonormal cores to 5e-5, approximation error within 2e-5 + 1e-2 relative of the oracle's."""
    import math

    import oracle

    one = [c[item].cpu() for c in inp]
    ref = oracle.round_tt([c.double() for c in one], rmax=R_OUT, algorithm="svd")
    ours = [c[item].cpu() for c in out.cores]

    def rel(a, b):
        a = [c.double() for c in a]
        b = [c.double() for c in b]
        aa, bb, ab = oracle.tt_dot(a, a), oracle.tt_dot(b, b), oracle.tt_dot(a, b)
        return math.sqrt(max((aa + bb - 2 * ab).item(), 0.0) / bb.item())

    e_o, e_r = rel(ours, one), rel(ref, one)
    sv = max(((a - b).abs().max() / b.max()).item()
             for a, b in zip(oracle.bond_singular_values(ours), oracle.bond_singular_values(ref)))
    orth = 0.0
    for c in ours[1:]:
        Rm = c.double().reshape(c.shape[0], -1)
        orth = max(orth, (Rm @ Rm.T - torch.eye(Rm.shape[0], dtype=torch.float64)).abs().max().item())
    ranks_ok = oracle.tt_ranks(ours) == oracle.tt_ranks(ref)
    # (approximation error: the fp32 bound of the headline's parity check -- 2e-5 through TT inner products at the metric size,
    # seven truncations in fp32 -- on top of the oracle's own error)
    ok = ranks_ok and sv <= 4e-6 and orth <= 5e-5 and abs(e_o - e_r) <= 2e-5 + 1e-2 * e_r
    return {"item": item, "ranks_identical": ranks_ok, "bond_sv_max_abs_diff_rel_sigma_max": sv, "right_orthonormality_defect": orth,
            "approx_err_ours": e_o, "approx_err_oracle_f64": e_r,
            "bounds": {"bond_sv": 4e-6, "orth": 5e-5, "approx_err_abs_diff": "2e-5 + 1e-2 * oracle"}, "ok": bool(ok)}


def kernel_model():
    """Algorithmic work of every kernel kind PER TENSOR of the metric workload (float32): `flops` = the arithmetic the
    kernel's algorithm performs, `bytes` = what it must move given its interface (operands read once, results written
    once, including the reflectors / T factors / R a factorisation leaves behind).  DESIGN.md section 3 lists them."""
    s = 4
    n, I, Rr, ro = R_IN, MODE, R_IN, R_OUT
    mid = N_CORES - 2                                  # cores 1..6: pushed 4096 x 64 factorisations
    m = Rr * I
    hh = lambda rows, cols: 2.0 * rows * cols * cols - 2.0 * cols ** 3 / 3.0      # Householder QR (factor only)
    leaf_blocks, leaf_rows = 8, 512
    # factor: level 0 = 8 blocks of 512 x 64 (+ the fused push R @ core), level 1 = one 512 x 64 block of stacked R's
    f_flops = mid * (leaf_blocks * hh(leaf_rows, n) + hh(leaf_blocks * n, n) + 2.0 * Rr * Rr * I * n) + hh(I, n)
    f_bytes = mid * s * (Rr * I * n            # core read
                         + m * n               # reflectors written (level 0)
                         + 2 * leaf_blocks * n * n + leaf_blocks * n * n   # stacked R written + read, level-1 reflectors
                         + 9 * 4 * 256 + n * n) + s * (I * n * 2)
    # apply: Q [C; 0] with C = U sigma (64 x 32): per level W = V^T C and C += V W2 over all reflector rows
    a_flops = mid * 4.0 * (m + leaf_blocks * n) * n * ro + 4.0 * I * n * ro
    a_bytes = mid * s * (m * n + leaf_blocks * n * n + m * ro + 2 * leaf_blocks * n * ro) + s * (I * n + I * ro)
    nb = I * ro                                        # right unfolding of a middle core: 64 x 2048
    bonds = [(Rr, nb)] * (N_CORES - 2) + [(Rr, I)]     # bond N-1 is 64 x 64
    sym = 10.0 / 16.0                                  # the Gram kernels compute 10 of the 16 tiles
    rg_flops = sum(2.0 * R * R * c * sym for R, c in bonds)
    rg_bytes = sum(s * R * c for R, c in bonds)
    ro_flops = sum(2.0 * R * R * c * (1 + sym) for R, c in bonds)
    pj_flops = sum(2.0 * R * ro * c for R, c in bonds)
    pj_bytes = sum(s * (R + ro) * c for R, c in bonds)
    eig_bytes = 2 * (N_CORES - 1) * s * 2 * Rr * Rr
    eig_flops = 2 * (N_CORES - 1) * 9.0 * Rr ** 3      # SURVEY 8d's 9 m^3 per eigenproblem
    gemm_flops = 2.0 * Rr * Rr * I                     # last-core push
    gemm_bytes = s * (Rr * Rr + 2 * Rr * I)
    return {
        "qr_factor": {"flops": f_flops, "bytes": f_bytes},
        "qr_apply": {"flops": a_flops, "bytes": a_bytes},
        "rowgram": {"flops": rg_flops, "bytes": rg_bytes},
        "rotgram": {"flops": ro_flops, "bytes": rg_bytes},
        "project": {"flops": pj_flops, "bytes": pj_bytes},
        "eigh": {"flops": eig_flops, "bytes": eig_bytes},
        "gemm": {"flops": gemm_flops, "bytes": gemm_bytes},
    }


CENSUS_KINDS = ("qr_factor", "qr_apply", "rowgram", "rotgram", "project", "gemm")   # kinds the library's census instruments


def per_kind_roofline(prof, work, B, steps, pmc=None, model=None):
    """Per kernel kind: device time (HIP events inside the library) against BOTH roofs, on the work the launches EXECUTED on this
    input (`_hip.prof_collect_work`: read off the kernels' own per-item / per-block decisions) -- `frac` is the larger of the two
    executed fractions and names the `bound`; the SURVEY-model (input-blind) figures stand beside it as `algorithmic` (their
    fractions can exceed 1 where a launch skips work the model prices: that is what "algorithmic" means, not a utilisation)."""
    model = model or kernel_model()
    out = {}
    for k, v in prof.items():
        if v["launches"] == 0:
            continue
        sec = v["ms"] * 1e-3
        entry = {"ms_per_step": v["ms"] / steps, "launches_per_step": v["launches"] / steps}
        if k in model:
            fl, by = model[k]["flops"] * B * steps, model[k]["bytes"] * B * steps
            entry["algorithmic"] = {"flops_per_step": fl / steps, "bytes_per_step": by / steps, "arithmetic_intensity": fl / by,
                                    "TFLOPs": fl / sec / 1e12, "GBs": by / sec / 1e9,
                                    "mfma_frac": fl / sec / 1e12 / MFMA_F32_PEAK_TF, "hbm_frac": by / sec / 1e9 / HBM_PEAK_GBS}
        w = (work or {}).get(k)
        if k in CENSUS_KINDS and w and (w["flops"] > 0 or w["bytes"] > 0):
            tf, gbs = w["flops"] / sec / 1e12, w["bytes"] / sec / 1e9
            ex = {"flops_per_step": w["flops"] / steps, "bytes_per_step": w["bytes"] / steps,
                  "arithmetic_intensity": w["flops"] / w["bytes"] if w["bytes"] > 0 else None,
                  "TFLOPs": tf, "GBs": gbs, "mfma_frac": tf / MFMA_F32_PEAK_TF, "hbm_frac": gbs / HBM_PEAK_GBS}
            entry["executed"] = ex
            entry["bound"] = "mfma" if ex["mfma_frac"] >= ex["hbm_frac"] else "hbm"
            entry["frac"] = max(ex["mfma_frac"], ex["hbm_frac"])
            if "algorithmic" in entry:
                entry["executed_share_of_algorithmic_flops"] = w["flops"] / (entry["algorithmic"]["flops_per_step"] * steps)
        elif k == "eigh":
            entry["bound"], entry["frac"] = "valu", None   # serial VALU chains (no MFMA roof applies); time only
        else:
            entry["bound"], entry["frac"] = None, None
        if pmc and k in pmc:
            sc = B / pmc.get("_batch", B)
            if pmc[k].get("hbm_bytes_per_step") is not None:
                entry["traffic_bytes_per_step"] = pmc[k]["hbm_bytes_per_step"] * sc
                entry["traffic_hbm_frac"] = entry["traffic_bytes_per_step"] / (entry["ms_per_step"] * 1e-3) / 1e9 / HBM_PEAK_GBS
            if pmc[k].get("mfma_util") is not None:
                entry["mfma_util"] = pmc[k]["mfma_util"]
        out[k] = entry
    return out


def sweep_executed(per_kind, ms_per_step):
    """The whole step on executed work: flops / bytes of the instrumented kinds over the step's wall time."""
    fl = sum(v["executed"]["flops_per_step"] for v in per_kind.values() if "executed" in v)
    by = sum(v["executed"]["bytes_per_step"] for v in per_kind.values() if "executed" in v)
    sec = ms_per_step * 1e-3
    return {"flops_per_step": fl, "bytes_per_step": by, "mfma_frac": fl / sec / 1e12 / MFMA_F32_PEAK_TF,
            "hbm_frac": by / sec / 1e9 / HBM_PEAK_GBS, "kinds": [k for k, v in per_kind.items() if "executed" in v]}


def headline_roofline(per_kind, dom, prof, steps, pmc_note=None):
    """`roofline` of the JSON line: the kind with the largest device time, on EXECUTED work (`frac`, `bound`), with the algorithmic
    (SURVEY-model) fraction on the same roof beside it, the counter traffic when profiles/pmc_latest.json describes this build."""
    d = per_kind[dom]
    launches = prof[dom]["launches"]
    ex, al = d.get("executed"), d.get("algorithmic") or {}
    bound = d.get("bound")
    if ex is None:   # (a kind the census does not cover dominates: time only)
        return {"kernel": dom, "bound": bound or "valu", "achieved": None, "peak": None, "unit": None, "frac": None, "traffic": None,
                "avg_launch_ms": prof[dom]["ms"] / launches, "launches": launches, "input_aware": False}
    if bound == "mfma":
        ach, peak, unit, f_al = ex["TFLOPs"], MFMA_F32_PEAK_TF, "TFLOP/s", al.get("mfma_frac")
    else:
        ach, peak, unit, f_al = ex["GBs"], HBM_PEAK_GBS, "GB/s", al.get("hbm_frac")
    traffic = d.get("traffic_bytes_per_step")
    return {
        "kernel": dom, "bound": bound, "achieved": ach, "peak": peak, "unit": unit, "frac": ach / peak,
        "frac_mfma_executed": ex["mfma_frac"], "frac_hbm_executed": ex["hbm_frac"], "frac_algorithmic": f_al,
        "frac_mfma_algorithmic": al.get("mfma_frac"), "frac_hbm_algorithmic": al.get("hbm_frac"),
        "executed_share_of_algorithmic_flops": d.get("executed_share_of_algorithmic_flops"),
        "traffic": None if traffic is None else traffic * steps / launches,
        "frac_hbm_traffic": d.get("traffic_hbm_frac"),
        "traffic_note": pmc_note if traffic is None else "FETCH_SIZE x2 + WRITE_SIZE per launch (profiles/pmc_latest.json, same kernel build)",
        "mfma_util": d.get("mfma_util"),
        "avg_launch_ms": prof[dom]["ms"] / launches, "launches": launches,
        "executed_flops_per_launch": ex["flops_per_step"] * steps / launches,
        "executed_bytes_per_launch": ex["bytes_per_step"] * steps / launches,
        "ridge_flop_per_byte": RIDGE, "input_aware": True,
    }


def source_sha(files=None):
    """Hash of the kernel sources: PMC numbers in profiles/pmc_latest.json only describe the build they were taken from.
    ``files``: restrict to these translation units (+ every header) -- see ``KIND_SOURCES``."""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "tntorch_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith(".h") or (f.endswith(".hip") and (files is None or f in files)):
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


# The translation unit(s) every kernel kind is compiled from (one object file each, tntorch_amd/csrc/Makefile): the counters of a
# kind stay valid as long as ITS sources (and the shared header) are byte-identical, whatever happens to the other files.
KIND_SOURCES = {
    "qr_factor": ["ttr_qr.hip"], "qr_apply": ["ttr_qr.hip"],
    "rowgram": ["ttr_sweep.hip"], "rotgram": ["ttr_sweep.hip"], "project": ["ttr_sweep.hip"],
    "eigh": ["ttr_eigh.hip"], "gemm": ["ttr_gemm.hip", "ttr_bjacobi.hip"], "misc": None,
}


def kind_shas():
    return {k: source_sha(v) for k, v in KIND_SOURCES.items()}


def load_pmc(path=None):
    """profiles/pmc_latest.json restricted to the kinds whose sources are unchanged since the counters were collected
    (``kind_sha``; files without it: all or nothing on ``source_sha``).  -> (dict or None, note or None)"""
    path = path or os.path.join(ROOT, "profiles", "pmc_latest.json")
    if not os.path.exists(path):
        return None, "no profiles/pmc_latest.json"
    try:
        pmc = json.load(open(path))
    except Exception as e:  # noqa: BLE001
        return None, f"unreadable pmc_latest.json: {e!r}"
    if pmc.get("source_sha") == source_sha():
        return pmc, None
    now, then = kind_shas(), pmc.get("kind_sha") or {}
    stale = sorted(k for k in KIND_SOURCES if k in pmc and then.get(k) != now[k])
    if len(stale) == sum(1 for k in KIND_SOURCES if k in pmc):
        print("bench.py: WARNING: profiles/pmc_latest.json was collected from a different kernel build "
              f"({pmc.get('source_sha')} != {source_sha()}): `traffic` / `mfma_util` are reported as null", file=sys.stderr)
        return None, "stale: collected from a different kernel build"
    for k in stale:
        del pmc[k]
    print(f"bench.py: note: counters of {stale} in profiles/pmc_latest.json predate a change of their sources and are not used",
          file=sys.stderr)
    return pmc, None


def cpu_baseline(budget_s=14.0):
    """Time the CPU oracle (restatement of the reference, same LAPACK calls) on a bounded sample.

    The reference's small-matrix LAPACK calls do not scale with threads (128 MKL threads are ~40x SLOWER
    than 8 on this workload), so a few thread counts are tried and the FASTEST is reported: the baseline
    is the best the CPU path can do on this box, not a strawman.
    """
    import oracle

    torch.manual_seed(0)
    g = oracle.tt_randn([MODE] * N_CORES, R_OUT, dtype=torch.float32)
    inp = oracle.tt_add(g, g)
    ncpu = os.cpu_count() or 8
    cands = sorted({t for t in (4, 8, 16, 32) if t <= ncpu})  # >32 MKL threads is minutes per tensor on this workload
    saved = torch.get_num_threads()
    t_start = time.perf_counter()
    best = {}
    trials = {}
    for alg in ("eig", "svd"):
        for nt in cands:
            if time.perf_counter() - t_start > budget_s * (0.5 if alg == "eig" else 1.0):
                break
            torch.set_num_threads(nt)
            oracle.round_tt(inp, rmax=R_OUT, algorithm=alg)  # warm-up (MKL init / thread pool)
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                oracle.round_tt(inp, rmax=R_OUT, algorithm=alg)
                ts.append(time.perf_counter() - t0)
                if ts[-1] > 1.5:
                    break
            med = sorted(ts)[len(ts) // 2]
            trials[f"{alg}@{nt}"] = med
            if alg not in best or med < best[alg][0]:
                best[alg] = (med, nt)
    torch.set_num_threads(saved)
    fast_alg = min(best, key=lambda a: best[a][0])
    sec, nt = best[fast_alg]
    return {
        "value": N_CORES / sec,
        "unit": "cores/s",
        "cores": nt,
        "kind": "port",
        "sample": f"oracle.round_tt(rmax=32) of ONE 64^8 rank-64 float32 TT (the metric's unit), median of <=3 runs per "
                  f"(algorithm, thread count) over threads {cands}; reported: fastest = algorithm='{fast_alg}' at {nt} threads.  "
                  "kind 'port': /root/reference does not travel to the GPU box; in the build container the reference itself takes "
                  "39 ms per tensor ('eig', 8 threads) against the oracle's 48 ms (same LAPACK calls, bit-identical output), "
                  "i.e. the port flatters the GPU by ~1.2x",
        "algorithm": fast_alg,
        # the port against the reference itself, measured in the build container (same LAPACK calls, bit-identical output; the
        # reference does not travel to the GPU box): reference = port / 1.2 per tensor, i.e. every "x CPU" figure of the port
        # overstates the reference by this factor -- `speedup_vs_reference_est` below is corrected
        "reference_factor": REFERENCE_FACTOR,
        "value_reference_est": N_CORES / sec * REFERENCE_FACTOR,
        "sec_per_tensor": {a: best[a][0] for a in best},
        "threads": {a: best[a][1] for a in best},
        "trials_sec": trials,
        "gflops": FLOP_PER_TENSOR / sec / 1e9,
    }


def parity_check(inp, out, items):
    """Items of the LAST timed step against the oracle's default algorithm (LAPACK gesdd, round.py:96): identical ranks,
    ||ours - oracle|| / ||oracle|| through float64 TT inner products (1e-5 in fp32, the bound of
    tests/test_gpu_parity.py::test_metric_config_two_stream_path_vs_oracle; measured 2.6e-6)."""
    import math

    import oracle

    worst, ranks_ok = 0.0, True
    for i in items:
        one = [c[i].cpu() for c in inp]
        ref = oracle.round_tt(one, rmax=R_OUT, algorithm="svd")
        ours = [c[i].cpu() for c in out.cores]
        ranks_ok = ranks_ok and oracle.tt_ranks(ours) == oracle.tt_ranks(ref)
        a = [c.double() for c in ours]
        b = [c.double() for c in ref]
        aa, bb, ab = oracle.tt_dot(a, a), oracle.tt_dot(b, b), oracle.tt_dot(a, b)
        worst = max(worst, math.sqrt(max((aa + bb - 2 * ab).item(), 0.0) / bb.item()))
    return {"items": list(items), "rel_err_vs_oracle_svd": worst, "ranks_identical": ranks_ok, "bound": 1e-5,
            "ok": bool(ranks_ok and worst <= 1e-5)}


LINE_LIMIT = 4096   # bytes of the ONE stdout line (round 4's 20.6 KB line was not parsed by the driver)
FULL_SIDECAR = os.path.join("profiles", "bench_full_latest.json")


def _r(x, nd=4):
    """Round floats for the compact line (significant digits, not decimals: 1.3e6 cores/s and 2.6e-6 errors both survive)."""
    if isinstance(x, bool) or not isinstance(x, float):
        return x
    if x != x or x in (float("inf"), float("-inf")):
        return None
    return float(f"{x:.{nd}g}")


def _pick(d, keys, nd=4):
    if not isinstance(d, dict):
        return {}
    out = {k: _r(d[k], nd) for k in keys if d.get(k) is not None}
    return {k: v for k, v in out.items() if v is not None}   # (NaN / Infinity round to None: dropped, never printed)


def compact_line(res, sidecar=True):
    """The ONE line bench.py prints (contract fields + `roofline` + `cpu_baseline` + one-number summaries); everything else
    -- `configs`, `extras`, `roofline_per_kernel`, per-step records -- goes to the sidecar ``FULL_SIDECAR`` and to stderr.
    A plain run's result has no `roofline` (no per-kernel pass) and writes no sidecar (``sidecar=False``): neither is named.
    tests/test_bench_cpu.py pins ``len(line) < LINE_LIMIT`` and the fields the driver checks."""
    out = {k: res.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                                   "scaling", "vs_baseline", "dtype", "data")}
    out["value"], out["ms_per_step"] = _r(out["value"], 7), _r(out["ms_per_step"], 6)
    out["config"] = _pick(res.get("config", {}), ("workload", "tensors_per_gpu_per_step", "algorithm", "streams_per_gpu", "parallelism"))
    ro = res.get("roofline")
    if ro is not None:
        out["roofline"] = _pick(ro, ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "frac_mfma_executed",
                                     "frac_hbm_executed", "frac_algorithmic", "executed_share_of_algorithmic_flops", "frac_hbm_traffic",
                                     "mfma_util", "avg_launch_ms", "launches", "input_aware"))
        out["roofline"].setdefault("traffic", None)
    cb = res.get("cpu_baseline")
    if cb:
        out["cpu_baseline"] = _pick(cb, ("value", "unit", "cores", "kind", "algorithm", "reference_factor"))
        out["cpu_baseline"]["sample"] = str(cb.get("sample", ""))[:160]
        out["speedup_vs_cpu_best"] = _r(res.get("speedup_vs_cpu_best"))
        out["speedup_vs_reference_est"] = _r(res.get("speedup_vs_reference_est"))
    if res.get("parity"):
        out["parity"] = _pick(res["parity"], ("ok", "rel_err_vs_oracle_svd", "ranks_identical", "bound", "error"))
    if res.get("nccl_ranks") is not None:
        out["nccl_ranks"] = res["nccl_ranks"]
    out["sweep"] = _pick(res, ("gflops", "whole_sweep_hbm_frac", "whole_sweep_frac_of_mfma_f32_peak", "tensors_per_s"))
    if isinstance(res.get("whole_sweep_executed"), dict):
        out["sweep"]["executed_hbm_frac"] = _r(res["whole_sweep_executed"].get("hbm_frac"))
        out["sweep"]["executed_mfma_frac"] = _r(res["whole_sweep_executed"].get("mfma_frac"))
    if isinstance(res.get("roofline_per_kernel"), dict):   # per kind: [bound, executed frac] (times: kernel_ms_per_step)
        out["kinds"] = {k: [v.get("bound"), _r(v.get("frac"), 3)] for k, v in res["roofline_per_kernel"].items()
                        if isinstance(v, dict) and v.get("frac") is not None}
    if res.get("kernel_ms_per_step"):
        out["kernel_ms_per_step"] = {k: _r(v, 3) for k, v in res["kernel_ms_per_step"].items()}
    if res.get("sweep_roofline"):
        out["sweep_roofline"] = {k: _pick(v, ("bound", "frac", "frac_algorithmic")) for k, v in res["sweep_roofline"].items()}
    if res.get("gather"):
        out["gather"] = _pick(res["gather"], ("mode", "collectives_in_timed_region", "alone_ms", "compute_only_ms_per_step", "predicted_speedup",
                                              "bytes_per_peer_per_step", "per_link_GBs", "hidden_under_compute"))
    ex = {}
    for k, v in (res.get("extras") or {}).items():
        if not isinstance(v, dict):
            continue
        e = _pick(v, ("ms_per_step", "cores_per_s", "speedup_vs_cpu_best", "speedup_vs_reference_est", "ms_per_call"))
        if "oracle_check" in v:
            e["ok"] = bool(v["oracle_check"].get("ok"))
        if "whole_sweep_hbm_frac" in v:
            e["hbm_frac"] = _r(v["whole_sweep_hbm_frac"], 3)
        if isinstance(v.get("dominant"), dict):
            e["dominant"] = [v["dominant"].get("kernel"), _r(v["dominant"].get("ms"), 3), _r(v["dominant"].get("frac"), 3)]
        if "error" in v:
            e["error"] = str(v["error"])[:80]
        ex[k] = e
    if ex:
        out["extras"] = ex
    cf = {}
    for k, v in (res.get("configs") or {}).items():
        if not isinstance(v, dict):
            continue
        e = _pick(v, ("ms", "ms_is"))
        r2 = v.get("roofline") or {}
        e.update(_pick(r2, ("bound", "frac")))
        if isinstance(v.get("oracle_check"), dict):
            e["ok"] = bool(v["oracle_check"].get("ok"))
        for sub, key in (("single_tensor", "ms"), ("lowrank_variant", "ms"), ("whole_config_on_one_gpu", "ms")):
            if isinstance(v.get(sub), dict) and key in v[sub]:
                e[f"{sub}_ms"] = _r(v[sub][key])
        if "speedup_vs_cpu" in v or "speedup_vs_cpu_extrapolated" in v:
            e["x_cpu"] = _r(v.get("speedup_vs_cpu", v.get("speedup_vs_cpu_extrapolated")), 3)
            if (v.get("cpu_baseline") or {}).get("kind") == "port":   # (the port is 1.2x slower than the reference: see cpu_baseline)
                e["x_ref_est"] = _r(e["x_cpu"] / REFERENCE_FACTOR, 3)
        if "error" in v:
            e["error"] = str(v["error"])[:80]
        cf[k] = e
    if cf:
        out["configs"] = cf
    if sidecar:
        out["full"] = FULL_SIDECAR
    line = json.dumps(out, allow_nan=False)
    # (belt and braces: a line above the limit loses its optional blocks, never its contract fields)
    for drop in ("kinds", "kernel_ms_per_step", "sweep_roofline", "extras", "configs", "gather", "sweep"):
        if len(line) < LINE_LIMIT:
            break
        out.pop(drop, None)
        line = json.dumps(out, allow_nan=False)
    assert len(line) < LINE_LIMIT, len(line)
    return line


def emit(res):
    """Full object -> sidecar (+ gpurun_out/ when it exists, + stderr); compact line -> stdout (the LAST line, flushed)."""
    full = json.dumps(res, default=str)
    for d in (os.path.join(ROOT, "profiles"), os.path.join(ROOT, "gpurun_out")):
        try:
            if os.path.isdir(d):
                with open(os.path.join(d, os.path.basename(FULL_SIDECAR)), "w") as f:
                    f.write(full + "\n")
        except OSError as e:  # (a read-only tree must not cost the line)
            print(f"bench.py: could not write {d}: {e!r}", file=sys.stderr)
    print("bench.py full result: " + full, file=sys.stderr)
    sys.stderr.flush()
    print(compact_line(res))
    sys.stdout.flush()


def emit_plain(res):
    """A plain run: the result object -> stderr, the compact line -> stdout (the LAST line, flushed); no sidecar is written."""
    print("bench.py result: " + json.dumps(res, default=str), file=sys.stderr)
    sys.stderr.flush()
    print(compact_line(res, sidecar=False))
    sys.stdout.flush()


def timed_steps(step, drain, fence, warmup, steps, on_timed_start=None):
    out = None
    for _ in range(warmup):
        # the result is held exactly as in the timed loop (the previous step's rounded train stays alive while the next step
        # runs): otherwise the second TIMED step is the first to need a second 3.3 GB result arena, and that hipMalloc stalls
        # the host for 0.3 ms on most boxes but ~95 ms on some (measured: step_ms [31.5, 32.3, 95.7, 31.6, ...] with
        # host_enqueue_ms 94.4 for that step = 44 instead of 31.6 ms/step over 5 steps).  `allocator` in the JSON line
        # reports the device allocations inside the timed region (0 with W >= 2).
        out = step()
    drain()
    fence()
    if on_timed_start is not None:
        on_timed_start()
    ms0 = torch.cuda.memory_stats()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = step()
    gathered = drain()  # every step's gather has completed inside the timed region
    fence()
    elapsed = time.perf_counter() - t0
    ms1 = torch.cuda.memory_stats()
    # device allocations INSIDE the timed region (hipMalloc of a multi-GB segment costs milliseconds): 0 in steady state
    timed_steps.allocator = {
        "device_allocs_in_timed_region": int(ms1.get("num_device_alloc", 0) - ms0.get("num_device_alloc", 0)),
        "device_frees_in_timed_region": int(ms1.get("num_device_free", 0) - ms0.get("num_device_free", 0)),
        "alloc_retries": int(ms1.get("num_alloc_retries", 0)),
        "reserved_GB_before": ms0.get("reserved_bytes.all.current", 0) / 1e9,
        "reserved_GB_after": ms1.get("reserved_bytes.all.current", 0) / 1e9,
    }
    return elapsed, out, gathered


DUMP_BUDGET = 60 * 10**6   # bytes of core data per --dump-outputs (64 MB in all with the .npy headers)


def dump_outputs(path, t):
    """The rounded cores of one step, as a caller receives them: core k of the sampled items -> path/core<k>.npy.  The sample
    is a fixed function of the batch size (seeded permutation, as many items as fit into DUMP_BUDGET, in batch order)."""
    import numpy as np

    B = t.cores[0].shape[0]
    per_item = sum(c[0].numel() * c.element_size() for c in t.cores)
    n = max(1, min(B, DUMP_BUDGET // per_item))
    idx = torch.randperm(B, generator=torch.Generator().manual_seed(0))[:n].sort().values
    os.makedirs(path, exist_ok=True)
    for k, c in enumerate(t.cores):
        np.save(os.path.join(path, f"core{k}.npy"), c.index_select(0, idx.to(c.device)).cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=4096,
                    help="tensors per GPU per step (4096: 26 GB of resident cores, ~90 GB with workspaces and two steps in flight; round 5 -- "
                         "rounds 1-4 ran 2048, still reported as `extras.batch_2048`: the launches' tails amortise better, +6 %%)")
    ap.add_argument("--algorithm", default="svd", choices=["svd", "eig"])
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: the per-kernel roofline pass, the parity check against the oracle, `extras`, `configs`, "
                         "the CPU baseline and (N > 1) the `gather` block, each in runs of its own after the timed steps; the full "
                         "result object goes to " + FULL_SIDECAR + ".  Without it a run times the steps and prints the line, nothing else")
    ap.add_argument("--config", default="metric", choices=["metric", "c1", "c2", "c3", "c4"],
                    help="metric (default): the headline workload (with --full its line also carries `configs`: one entry per BASELINE config); "
                         "c1 .. c4: one of BASELINE's other configs alone (tools/bench_configs.py)")
    ap.add_argument("--variant", default="randn", choices=["randn", "lowrank"],
                    help="--config c1 | c3: the input of SURVEY 8d (plain randn, or TT rank = the cap of unit RMS + 1e-3 randn)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-extras", action="store_true", help="--full: skip the small-batch / single-tensor extra measurements")
    ap.add_argument("--no-configs", action="store_true", help="--full: skip the C1 .. C4 entries of the line (`configs`)")
    ap.add_argument("--gather", default=os.environ.get("TTR_BENCH_GATHER", "end"), choices=["end", "step", "none"],
                    help="N > 1: `end` (default; north_star: 'a single RCCL gather over xGMI at the end') = ONE gather of the last "
                         "step's rounded cores after the last timed step, inside the timed region; `step` = every step's result is "
                         "gathered on rank 0 (asynchronously, under the next step's compute: link-bound at 8 GPUs, DESIGN section 9); "
                         "`none` = no gather (compute-only scaling)")
    ap.add_argument("--single-stream", action="store_true",
                    help="issue the timed region on one stream too (for rocprofv3 kernel traces: with sub-batch "
                         "streams the traced kernel durations overlap)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the rounded cores of the last step as DIR/core<k>.npy (float32, "
                         "[items, r_k, 64, r_k+1]) for a fixed seeded sample of the batch items, at most 64 MB in all (rank 0's batch)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs is not None and args.config != "metric":
        ap.error("--dump-outputs: the metric workload only")
    if args.config != "metric":
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import bench_configs
        return bench_configs.main(args)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: start the N ranks ourselves (one process per GPU, torch.distributed.run with the
        # loopback rendezvous the driver would use); rank 0 of the child job prints the JSON line
        import socket
        import subprocess

        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        return sys.exit(subprocess.call(cmd, env=env))

    import torch.distributed as dist

    import tntorch_amd as tn
    from tntorch_amd import _hip
    from tntorch_amd.dist_batch import GatherSchedule, gather_batch

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} needs a torch.distributed.run launch with WORLD_SIZE={args.gpus}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the HIP path has no CPU fallback)")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    nccl_ranks = 1
    # TTR_BENCH_FORCE_DIST=1 (tests, under torch.distributed.run with ONE rank): the N > 1 code path -- process group, gather
    # schedule through the real collective, barriers, max-over-ranks -- on a single GPU
    dist_on = world > 1 or (os.environ.get("TTR_BENCH_FORCE_DIST") == "1" and "RANK" in os.environ)
    if dist_on:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        nccl_ranks = dist.get_world_size()
    _hip.lib()  # fail loudly if the kernels are not built
    from tntorch_amd import _hipops
    if args.single_stream:
        _hipops.STREAM_CHUNKS_ENABLED = False

    B = args.batch
    inp = make_input(B, dev, seed=1234 + rank)

    sizes = [B] * world
    sched = GatherSchedule(args.gather if dist_on else "none", sizes=sizes, dst=0, local_shortcut=not dist_on)
    # N > 1: the steps are issued from a stream of their own instead of the default stream.  Measured on one GPU
    # (tools/probes/dist_overhead_probe.py, profiles/r05_dist_overhead.txt): with a live RCCL communicator the same step costs
    # 27.3 - 27.4 ms instead of 24.8 - 25.0 when it is enqueued from the default stream (destroying the process group restores
    # it; gloo and a lazily initialised nccl group cost nothing), and 24.95 ms from a (high-priority) stream of its own.
    work_stream = torch.cuda.Stream(device=dev, priority=-1) if (dist_on and os.environ.get("TTR_BENCH_WORK_STREAM", "1") != "0") else None

    if work_stream is not None:   # (`inp` was produced on the default stream)
        work_stream.wait_stream(torch.cuda.current_stream())

    def on_work_stream():
        return torch.cuda.stream(work_stream) if work_stream is not None else contextlib.nullcontext()
    inflight = []  # completion events of the steps enqueued so far
    step_events = []  # all of them, for the per-step device times reported in the JSON line
    host_ms = []      # host time spent enqueuing each step

    def step():
        """Round the local batch; for N > 1 hand the rounded cores to the (asynchronous) gather.  The gather
        of step k runs on RCCL's stream under the compute of step k+1; at most one gather is in flight.
        The host runs at most two steps ahead of the device (enqueuing a step costs < 1 ms of host time): with an
        unbounded run-ahead every step in flight holds its own ~30 GB of QR workspaces, and the first process on a
        fresh box then spends the timed region in hipMalloc (measured: 49 instead of 38 ms per step)."""
        if len(inflight) >= int(os.environ.get("TTR_BENCH_RUNAHEAD", "2")):
            inflight.pop(0).synchronize()
        h0 = time.perf_counter()
        with on_work_stream():
            t = tn.Tensor(inp, batch=True)
            t.round_tt(rmax=R_OUT, algorithm=args.algorithm)
            host_ms.append(round((time.perf_counter() - h0) * 1e3, 2))
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            inflight.append(ev)
            step_events.append(ev)
            sched.after_step(t)   # `step`: start this step's gather (after the previous one completed); `end` / `none`: nothing moves
        return t

    def drain():
        """Everything the root is owed has arrived when this returns (called inside the timed region): `end` = THE gather."""
        with on_work_stream():   # (the collective orders itself behind the stream that produced the cores)
            return sched.drain()

    def fence():
        torch.cuda.synchronize()
        if dist_on:
            dist.barrier()
            torch.cuda.synchronize()

    elapsed, out, gathered = timed_steps(step, drain, fence, args.warmup, args.steps, on_timed_start=lambda: setattr(sched, "g0", sched.gathers))
    sched.gathers_timed = sched.gathers - getattr(sched, "g0", 0)
    if args.dump_outputs is not None and rank == 0:
        dump_outputs(args.dump_outputs, out)
    if dist_on:
        tt = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
        if rank == 0 and args.gather != "none":  # the root really holds every rank's rounded cores
            assert gathered is not None and len(gathered) == world
            assert all(list(g.ranks_tt) == [1] + [R_OUT] * (N_CORES - 1) + [1] and g.cores[0].shape[0] == B for g in gathered)
            assert torch.isfinite(gathered[-1].cores[3]).all()

    # ---- N > 1: the gather of one step's result ALONE (nothing else running), so that a scaling line shows which side
    # binds: `gather.alone_ms` against `ms_per_step`.  Every peer sends its packed cores over its own xGMI link to rank 0.  --full only.
    gather_info = None
    if dist_on and args.full:
        per_peer = sum(c.numel() * c.element_size() for c in out.cores)
        fence()
        g0 = time.perf_counter()
        with on_work_stream():
            gather_batch(out, dst=0, sizes=sizes, async_op=False, local_shortcut=False).wait()
        fence()
        g_ms = (time.perf_counter() - g0) * 1e3
        # ... and the steps ALONE (no gather at all), same fences: with `end` the timed region is steps * compute_only + one gather
        mode_saved, sched.mode = sched.mode, "none"
        n_ev, n_h = len(step_events), len(host_ms)
        fence()
        c0 = time.perf_counter()
        for _ in range(min(args.steps, 3)):
            step()
        fence()
        c_ms = (time.perf_counter() - c0) * 1e3 / min(args.steps, 3)
        sched.mode = mode_saved
        del step_events[n_ev:], host_ms[n_h:]   # (not part of the timed region's per-step records)
        free_b, total_b = torch.cuda.mem_get_info()
        # the model a SCALE record can be checked against: N ranks, K steps of c ms compute each and -- `end` -- one gather of g ms
        # at the end: speedup over one GPU = N K c / (K c + g); `step`: N c / max(c, g); `none`: N
        _K, _c, _g, _N = args.steps, c_ms, g_ms, world
        predicted = {"end": _N * _K * _c / (_K * _c + _g), "step": _N * _c / max(_c, _g), "none": float(_N)}[args.gather]
        gather_info = {"mode": args.gather, "collectives_in_timed_region": sched.gathers_timed, "bytes_per_peer_per_step": per_peer,
                       "predicted_speedup": predicted,
                       "predicted_speedup_model": "N K c / (K c + alone_ms) for `end`; N c / max(c, alone_ms) for `step`; c = compute_only_ms_per_step",
                       "peers": world - 1, "alone_ms": g_ms, "compute_only_ms_per_step": c_ms,
                       "steps_on_own_stream": work_stream is not None,
                       # `step`: the gather of step k has to hide under the compute of step k + 1 -- if it does not, the job is link-bound
                       "hidden_under_compute": bool(g_ms < c_ms) if args.gather == "step" else None,
                       "root_inbound_GBs": per_peer * max(world - 1, 1) / g_ms / 1e6, "per_link_GBs": per_peer / g_ms / 1e6,
                       "root_receive_buffers_GB": per_peer * world / 1e9 * (2 if args.gather == "step" else 1),
                       "hbm_GB": {"total": total_b / 1e9, "free_now": free_b / 1e9,
                                  "reserved_by_torch": torch.cuda.memory_reserved() / 1e9}}

    # ---- per-kernel device time over an identical pass (HIP events on the launch stream).  The timed region
    # above runs sub-batches on several streams so that kernels overlap; here every kernel must run alone for
    # its duration to mean anything, so the same work is issued on ONE stream.  --full only.
    if args.full:
        _hipops.STREAM_CHUNKS_ENABLED = False
        # (one untimed step first: this is the first time these kernels run on THIS stream's queue -- the runtime sizes a queue's
        # scratch memory when a kernel first needs it there, a one-off stall of tens of milliseconds that landed in the `eigh` kind of
        # some runs: 8.1 instead of 1.5 ms/step averaged over 20 steps, with the timed region of the same process at 13.7 ms/step)
        t = tn.Tensor(inp, batch=True)
        t.round_tt(rmax=R_OUT, algorithm=args.algorithm)
        torch.cuda.synchronize()
        _hip.prof_enable(2)   # per-kind device times + the executed-work census (include/ttround_hip.h: ttr_prof_collect_work)
        for _ in range(args.steps):
            t = tn.Tensor(inp, batch=True)
            t.round_tt(rmax=R_OUT, algorithm=args.algorithm)
        torch.cuda.synchronize()
        prof = _hip.prof_collect()
        work = _hip.prof_collect_work()
        _hip.prof_enable(False)
        _hipops.STREAM_CHUNKS_ENABLED = not args.single_stream

    if rank == 0:
        assert list(out.ranks_tt) == [1] + [R_OUT] * (N_CORES - 1) + [1], out.ranks_tt
        tensors = B * world * args.steps
        ms_per_step = elapsed / args.steps * 1e3
        cores_per_s = tensors * N_CORES / elapsed
        res = {
            "metric": f"TT rounding 64^8 rank-64 -> rank-32 (round_tt rmax=32), cores/s, resident batch of {B} trains per GPU",
            "value": cores_per_s,
            "unit": "cores/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {
                "workload": "round_tt(rmax=32) of 64^8 TT tensors, rank 64 (g+g, g randn rank 32), fp32, batch-resident in HBM",
                "tensors_per_gpu_per_step": B,
                "algorithm": args.algorithm,
                "streams_per_gpu": 1 if args.single_stream else 2,
                "parallelism": (f"batch-sharded x{world}, " + {
                    "step": "one async RCCL gather of packed cores per step (overlapped with the next step)",
                    "end": "ONE RCCL gather of the packed cores after the last step (inside the timed region)",
                    "none": "no gather"}[args.gather]) if dist_on else "single GPU",
            },
            # data-dependent shortcuts that fire on this input (all decided per item on the device; knobs: include/ttround_hip.h)
            "shortcuts": {
                "input_structure": "t = g + g: every unfolding / R factor has numerical rank 32 of 64",
                "qr_rank_skip": "panels whose remaining part is below 8 eps of their block are H = I (TTR_KNOB_QR_RANK_SKIP): 2 of 4 panels per block",
                "qr_row_packing": "R factors of numerical rank <= 32: two mode indices per wave, half the level-0 blocks, block-major launch (TTR_KNOB_QR_PACK = 3)",
                "rows32": "the carry of a packed bond has exactly zero rows 32..: not written by the apply, not loaded by rowgram / rotgram / project",
                "flat_spectrum": "kept singular values within a factor 8: pass 2 skipped, pass 1 by the top-r solver",
            },
            "nccl_ranks": nccl_ranks,
            "allocator": getattr(timed_steps, "allocator", None),
            # device time between the completion events of consecutive steps (warm-up steps included, first one omitted)
            "host_enqueue_ms": host_ms,
            "step_ms": [round(step_events[i - 1].elapsed_time(step_events[i]), 2) for i in range(1, len(step_events))],
            "tensors_per_s": tensors / elapsed,
            "gflops": FLOP_PER_TENSOR * tensors / elapsed / 1e9,
            "whole_sweep_frac_of_mfma_f32_peak": FLOP_PER_TENSOR * tensors / elapsed / 1e12 / MFMA_F32_PEAK_TF,
            "whole_sweep_hbm_frac": BYTES_PER_TENSOR * tensors / elapsed / 1e9 / HBM_PEAK_GBS,
        }
        if not args.full:
            emit_plain(res)
    if rank == 0 and args.full:
        pmc, pmc_note = load_pmc()
        per_kind = per_kind_roofline(prof, work, B, args.steps, pmc)
        dom = max(per_kind, key=lambda k: per_kind[k]["ms_per_step"])
        res.update({
            "gather": gather_info,
            "whole_sweep_executed": sweep_executed(per_kind, ms_per_step),
            "roofline": headline_roofline(per_kind, dom, prof, args.steps, pmc_note),
            "roofline_per_kernel": per_kind,
            "kernel_ms_per_step": {k: v["ms"] / args.steps for k, v in prof.items() if v["launches"] > 0},
        })
        try:
            res["parity"] = parity_check(inp, out, (0, B - 1) if B > 1 else (0,))
        except Exception as e:  # noqa: BLE001
            res["parity"] = {"ok": False, "error": repr(e)}
        if world == 1 and not args.no_extras:
            extras = {}
            for Bx, label, st in ((64, "batch_64", 10), (1, "single_tensor", 20)):
                if Bx >= B:
                    continue
                small = [c[:Bx].contiguous() for c in inp]

                def sstep(small=small):
                    t = tn.Tensor(small, batch=True)
                    t.round_tt(rmax=R_OUT, algorithm=args.algorithm)
                    return t
                # (fastest of three timed blocks: a step of a few ms is enqueue-bound on the host, and one disturbed block -- the
                # parity check's LAPACK threads winding down -- moved the figure by 50 % between otherwise identical runs)
                el = min(timed_steps(sstep, lambda: None, torch.cuda.synchronize, 3, st)[0] for _ in range(3))
                extras[label] = {"tensors_per_step": Bx, "ms_per_step": el / st * 1e3, "cores_per_s": Bx * N_CORES * st / el}
            # (nothing of the small-batch runs may stay alive: a 1 MB core of `small` pins the multi-GB segment the caching allocator
            # carved it from, and config C1 at 64^6 needs all but 5 GiB of the device -- round 5's first B = 4096 run fell back to 48 x 64^5)
            small = sstep = None
            for Bo in (2048,):
                # other resident batches: what rounds 1-4 reported (2048: the launches' tails weigh more)
                if Bo == B or B != 4096:
                    continue
                try:
                    big = make_input(Bo, dev, seed=4321)

                    def bstep(big=big):
                        t = tn.Tensor(big, batch=True)
                        t.round_tt(rmax=R_OUT, algorithm=args.algorithm)
                        return t
                    el, _, _ = timed_steps(bstep, lambda: None, torch.cuda.synchronize, 2, 5)
                    extras[f"batch_{Bo}"] = {"tensors_per_step": Bo, "ms_per_step": el / 5 * 1e3, "cores_per_s": Bo * N_CORES * 5 / el}
                    del big, bstep   # (the closure's default argument holds the input too)
                except Exception as e:  # noqa: BLE001
                    extras[f"batch_{Bo}"] = {"error": repr(e)[:200]}
                torch.cuda.empty_cache()
            # SURVEY 8d's second variant of the metric input: bond singular values ~ 2^(-decay j).  Every shortcut that makes the
            # flat `randn`-core input fast declines here (the second Gram pass runs, the first pass is the full QL solver);
            # same shapes, same B, checked against the float64 oracle.
            for decay in (1.0, 0.5):
                try:
                    dinp = make_decaying_input(B, dev, seed=777, decay=decay)

                    def dstep(dinp=dinp):
                        t = tn.Tensor(dinp, batch=True)
                        t.round_tt(rmax=R_OUT, algorithm=args.algorithm)
                        return t
                    el, dout, _ = timed_steps(dstep, lambda: None, torch.cuda.synchronize, 2, 5)
                    ent = {"tensors_per_step": B, "bond_sigma": f"~2^(-{decay} j)", "ms_per_step": el / 5 * 1e3,
                           "cores_per_s": B * N_CORES * 5 / el, "ratio_to_headline": (el / 5 * 1e3) / ms_per_step}
                    _hipops.STREAM_CHUNKS_ENABLED = False
                    dstep()   # (untimed: first use of this input's kernels on the single stream, see the headline's pass)
                    torch.cuda.synchronize()
                    _hip.prof_enable(2)
                    dstep()
                    torch.cuda.synchronize()
                    pk = _hip.prof_collect()
                    wk = _hip.prof_collect_work()
                    _hip.prof_enable(False)
                    _hipops.STREAM_CHUNKS_ENABLED = not args.single_stream
                    ent["kernel_ms_per_step"] = {k: round(v["ms"], 3) for k, v in pk.items() if v["launches"] > 0}
                    pkr = per_kind_roofline(pk, wk, B, 1)
                    ent["roofline_per_kernel"] = pkr
                    ent["whole_sweep_executed"] = sweep_executed(pkr, ent["ms_per_step"])
                    ent["whole_sweep_hbm_frac"] = BYTES_PER_TENSOR * B / (ent["ms_per_step"] * 1e-3) / 1e9 / HBM_PEAK_GBS
                    dk = max(pkr, key=lambda k: pkr[k]["ms_per_step"])
                    ent["dominant"] = {"kernel": dk, "ms": pkr[dk]["ms_per_step"], "bound": pkr[dk].get("bound"), "frac": pkr[dk].get("frac")}
                    ent["oracle_check"] = decaying_parity(dinp, dout, 0)
                    extras[f"decaying_spectrum_{decay}"] = ent
                    del dinp, dout, dstep   # (the closure's default argument holds the input too)
                except Exception as e:  # noqa: BLE001
                    extras[f"decaying_spectrum_{decay}"] = {"error": repr(e)[:300]}
                torch.cuda.empty_cache()
            res["extras"] = extras
        if world == 1 and not args.no_extras and not args.no_configs:
            # BASELINE's other configs (C1 .. C4), one entry each: time, SURVEY 8d flops / bytes, roofline fraction, CPU
            # baseline on the config or its largest feasible proxy, oracle check (tools/bench_configs.py)
            del inp, out, t
            sched._last = None          # (everything that still holds a step's result: C1 needs the whole device)
            inflight.clear()
            step_events.clear()
            gathered = None
            import gc
            gc.collect()
            torch.cuda.empty_cache()
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import bench_configs
            res["configs"] = bench_configs.config_extras(tn, dev, algorithm=args.algorithm, cpu=not args.no_cpu_baseline)
        if world == 1 and not args.no_cpu_baseline:
            cb = cpu_baseline()
            res["cpu_baseline"] = cb
            res["speedup_vs_cpu_best"] = cores_per_s / cb["value"]
            res["speedup_vs_reference_est"] = cores_per_s / cb["value_reference_est"]
            if "extras" in res and "single_tensor" in res["extras"]:
                res["extras"]["single_tensor"]["speedup_vs_cpu_best"] = res["extras"]["single_tensor"]["cores_per_s"] / cb["value"]
                res["extras"]["single_tensor"]["speedup_vs_reference_est"] = res["extras"]["single_tensor"]["cores_per_s"] / cb["value_reference_est"]
        emit(res)
    if dist_on:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

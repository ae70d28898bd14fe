"""The refusals of the C ABI, pinned on a CPU-only box: status code and ``ttr_last_error()`` text of every argument check that
the entries of the feature units take from the shared host helpers (csrc/detail/ttr_internal.h).

An entry's checks return before anything touches a device, so the library is called through ``ctypes`` with the addresses of
small HOST arrays; nothing dereferences them before the refusal.  With a GPU visible the module is skipped: a host address
must never reach a launch on a real device.  Without one, a check that wrongly passes ends in a HIP "no device" status and the
case fails.  The expectations were recorded from the library as it was BEFORE the helpers were merged."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="host addresses must not reach a launch on a real device")

F32, F64 = 0, 1
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
R, I, C = 3, 5, 7

_BUF = [(ctypes.c_double * 512)() for _ in range(6)]
A0, A1, A2, A3, A4, A5 = (ctypes.addressof(b) for b in _BUF)


def i64(values):
    return None if values is None else (ctypes.c_int64 * len(values))(*values)


def ptrs(values):
    return None if values is None else (ctypes.c_void_p * len(values))(*values)


XS = (I * C, C, 1)   # the strides of a contiguous [R, I, C]
BIG = 1 << 21        # BIG^3 elements leave the index envelope


def mode_diff(dtype=F32, R=R, I=I, C=C, order=1, X=A0, xs=XS, Y=A1, ys=XS):
    return "ttr_mode_diff", (dtype, R, I, C, order, 0, 1.0, X, i64(xs), Y, i64(ys), None)


def laplace_core(dtype=F32, R=R, I=I, C=C, pos=1, X=A0, xs=XS, out=A1):
    return "ttr_laplace_core", (dtype, R, I, C, pos, 0, 1.0, X, i64(xs), out, None)


def mode_scan(dtype=F32, R=R, I=I, C=C, X=A0, xs=XS, Y=A1, ys=XS):
    return "ttr_mode_scan", (dtype, R, I, C, X, i64(xs), Y, i64(ys), None)


def mode_reduce(dtype=F32, R=R, I=I, C=C, X=A0, xs=XS, w=A2, Y=A1, ys=(C, 1)):
    return "ttr_mode_reduce", (dtype, R, I, C, X, i64(xs), w, 1.0, Y, i64(ys), None)


def core_matvec(dtype=F32, P=2, K=I, Q=3, A=R, S=4, C=C, x=A0, xs=(I * 3, 3, 1), G=A1, gs=(I * 4 * C, 4 * C, C, 1), out=A2):
    return "ttr_core_matvec", (dtype, P, K, Q, A, S, C, x, i64(xs), G, i64(gs), out, None)


def hsum_step(dtype=F32, K=2, I=I, rin=(3, 4), rout=(2, 6), W=A0, cores=(A1, A2), cs=(10, 2, 1, 30, 6, 1), Wout=A3, ws=A4, wsb=1 << 20):
    return "ttr_hsum_step", (dtype, K, I, i64(rin), i64(rout), W, ptrs(cores), i64(cs), Wout, ws, wsb, None)


def hsum_bytes(dtype=F32, K=2, I=I, rin=(3, 4), rout=(2, 6)):
    return "ttr_hsum_step_workspace_bytes", (dtype, K, I, i64(rin), i64(rout))


def sandwich(dtype=F32, S=2, R=R, I=20, C=C, Z=A0, A=A1, as_=(20 * C, C, 1), w=A2, mu=A3, Q=A4, ws=A5, wsb=1 << 20):
    return "ttr_mode_sandwich", (dtype, S, R, I, C, Z, A, i64(as_), w, mu, Q, ws, wsb, None)


def convolve(dtype=F32, R1=2, I=I, R2=3, S1=2, J=4, S2=3, lo=0, K=8, a=A0, c=A1, out=A2):
    return "ttr_core_convolve", (dtype, R1, I, R2, S1, J, S2, lo, K, a, c, out, None)


def bad_dtype(name):
    """dtype 7 and nothing else: zeros and null pointers, as the parsed signature asks for them"""
    from tntorch_amd import _hip

    zero = {ctypes.c_int: 0, ctypes.c_int64: 0, ctypes.c_double: 0.0}
    return name, (7,) + tuple(zero.get(t) for t in _hip._SIGNATURES[name][1][1:])


def core_cases(entry, out, out_name):
    """the six checks every entry on a contiguous core [R, I, C] shares; `out`: the keyword of the entry's output pointer"""
    who = entry()[0]
    return [
        (entry(dtype=7), INVALID, f"{who}: bad dtype 7"),
        (entry(R=0), INVALID, f"{who}: bad sizes R = 0, I = 5, C = 7"),
        (entry(I=-1), INVALID, f"{who}: bad sizes R = 3, I = -1, C = 7"),
        (entry(C=0), INVALID, f"{who}: bad sizes R = 3, I = 5, C = 0"),
        (entry(X=None), INVALID, f"{who}: null pointer"),
        (entry(xs=None), INVALID, f"{who}: null pointer"),
        (entry(**{out: None}), INVALID, f"{who}: null pointer"),
        (entry(**{out: A0}), INVALID, f"{who}: X and {out_name} must be different buffers"),
        (entry(xs=(1, R, R * I)), UNSUPPORTED, f"{who}: X must be contiguous"),
        (entry(xs=(I * C, C, 2)), UNSUPPORTED, f"{who}: X must be contiguous"),
        (entry(R=BIG, I=BIG, C=BIG, xs=(BIG * BIG, BIG, 1)), UNSUPPORTED, f"{who}: core too large"),
        (entry(R=1, I=1 << 40, C=1 << 40, xs=(-3, 1 << 40, 1)), UNSUPPORTED, f"{who}: core too large"),   # an extent-1 stride is free
    ]


def strided_y_cases(entry):
    who = entry()[0]
    text = f"{who}: Y needs element strides (sr, si, 1) with si >= C and sr >= I si"
    return [
        (entry(ys=(I * C, C, 2)), UNSUPPORTED, text),
        (entry(ys=(I * C, C - 1, 1)), UNSUPPORTED, text),
        (entry(ys=(I * C - 1, C, 1)), UNSUPPORTED, text),
        (entry(ys=(I * (C + 1) - 1, C + 1, 1)), UNSUPPORTED, text),
        (entry(R=1, ys=(0, C - 1, 1)), UNSUPPORTED, text),          # R = 1: sr is free, si is not
        (entry(ys=(1 << 56, C, 1)), UNSUPPORTED, f"{who}: Y too large"),
    ]


CASES = (
    core_cases(mode_diff, "Y", "the output")
    + [
        (mode_diff(ys=None), INVALID, "ttr_mode_diff: null pointer"),
        (mode_diff(Y=A0, ys=None), INVALID, "ttr_mode_diff: X and the output must be different buffers"),  # the buffers come first
        (mode_diff(order=0), INVALID, "ttr_mode_diff: order 0 < 1"),
        (mode_diff(order=5), UNSUPPORTED, "ttr_mode_diff: order 5 above the fused limit 4 (chain calls)"),
        (mode_diff(order=0, ys=(I * C, C, 2)), INVALID, "ttr_mode_diff: order 0 < 1"),                     # the order before Y's strides
    ]
    + strided_y_cases(mode_diff)
    + core_cases(laplace_core, "out", "the output")
    + [
        (laplace_core(pos=3), INVALID, "ttr_laplace_core: pos 3 is none of 0 (first), 1 (middle), 2 (last)"),
        (laplace_core(pos=-1), INVALID, "ttr_laplace_core: pos -1 is none of 0 (first), 1 (middle), 2 (last)"),
    ]
    + core_cases(mode_scan, "Y", "Y")
    + [
        (mode_scan(ys=None), INVALID, "ttr_mode_scan: null pointer"),
        (mode_scan(Y=A0, ys=None), INVALID, "ttr_mode_scan: null pointer"),                                # the pointers come first
    ]
    + strided_y_cases(mode_scan)
    + core_cases(mode_reduce, "Y", "Y")
    + [
        (mode_reduce(ys=None), INVALID, "ttr_mode_reduce: null pointer"),
        (mode_reduce(Y=A0, ys=None), INVALID, "ttr_mode_reduce: null pointer"),
        (mode_reduce(w=A1), INVALID, "ttr_mode_reduce: w and Y must be different buffers"),
        (mode_reduce(ys=(C, 2)), UNSUPPORTED, "ttr_mode_reduce: Y needs element strides (sr, 1) with sr >= C"),
        (mode_reduce(ys=(C - 1, 1)), UNSUPPORTED, "ttr_mode_reduce: Y needs element strides (sr, 1) with sr >= C"),
        (mode_reduce(ys=(1 << 56, 1)), UNSUPPORTED, "ttr_mode_reduce: Y too large"),
    ]
    + [
        (core_matvec(dtype=7), INVALID, "ttr_core_matvec: bad dtype 7"),
        (core_matvec(P=0), INVALID, "ttr_core_matvec: bad sizes"),
        (core_matvec(C=0), INVALID, "ttr_core_matvec: bad sizes"),
        (core_matvec(x=None), INVALID, "ttr_core_matvec: null pointer"),
        (core_matvec(gs=None), INVALID, "ttr_core_matvec: null pointer"),
        (core_matvec(out=None), INVALID, "ttr_core_matvec: null pointer"),
        (core_matvec(xs=(1, 2, 2 * I)), UNSUPPORTED, "ttr_core_matvec: x and G must be contiguous"),
        (core_matvec(gs=(I * 4 * C, 4 * C, C, 2)), UNSUPPORTED, "ttr_core_matvec: x and G must be contiguous"),
        (core_matvec(P=BIG, K=BIG, Q=BIG, xs=(BIG * BIG, BIG, 1), gs=(BIG * 4 * C, 4 * C, C, 1)), UNSUPPORTED,
         "ttr_core_matvec: core too large"),
    ]
    + [
        (hsum_step(dtype=7), INVALID, "ttr_hsum_step: bad dtype 7"),
        (hsum_bytes(dtype=7), INVALID, "ttr_hsum_step: bad dtype 7"),
        (hsum_step(K=0), INVALID, "ttr_hsum_step: bad sizes"),
        (hsum_step(rin=None), INVALID, "ttr_hsum_step: bad sizes"),
        (hsum_step(K=9, rin=(2,) * 9, rout=(2,) * 9), UNSUPPORTED, "ttr_hsum_step: K = 9 > 8"),
        (hsum_step(rin=(3, 0)), INVALID, "ttr_hsum_step: rank < 1"),
        (hsum_step(rin=(3, 1 << 30)), UNSUPPORTED, "ttr_hsum_step: core too large"),
        (hsum_step(I=1, rin=(1 << 16, 1 << 16)), UNSUPPORTED, "ttr_hsum_step: prod(ranks) above 2^31 - 1"),
        (hsum_step(rin=(2, 40000), rout=(40000, 2)), UNSUPPORTED,
         "ttr_hsum_step: the intermediates of these ranks need more than 4294967296 bytes of scratch"),
        (hsum_step(W=None), INVALID, "ttr_hsum_step: null pointer"),
        (hsum_step(cs=None), INVALID, "ttr_hsum_step: null pointer"),
        (hsum_step(cores=(A1, None)), INVALID, "ttr_hsum_step: null core 1"),
        (hsum_step(cs=(10, 2, 1, 30, 6, 2)), UNSUPPORTED, "ttr_hsum_step: core 1 is not contiguous"),
        (hsum_step(cs=(1, 3, 15, 30, 6, 1)), UNSUPPORTED, "ttr_hsum_step: core 0 is not contiguous"),
        (hsum_step(wsb=0), WORKSPACE, "ttr_hsum_step: workspace 0 < 512 bytes"),
        (hsum_step(dtype=F64, wsb=511), WORKSPACE, "ttr_hsum_step: workspace 511 < 1024 bytes"),
        (hsum_step(ws=None), WORKSPACE, "ttr_hsum_step: workspace 1048576 < 512 bytes"),
    ]
    + [
        (sandwich(dtype=7), INVALID, "ttr_mode_sandwich: bad dtype 7"),
        (bad_dtype("ttr_mode_sandwich_workspace_bytes"), INVALID, "ttr_mode_sandwich: bad dtype 7"),
        (sandwich(S=0), INVALID, "ttr_mode_sandwich: bad sizes S = 0, R = 3, I = 20, C = 7"),
        (sandwich(R=65), UNSUPPORTED, "ttr_mode_sandwich: ranks 65 x 7 above 64"),
        (sandwich(S=65536), UNSUPPORTED, "ttr_mode_sandwich: S = 65536 > 65535"),
        (sandwich(I=1 << 45), UNSUPPORTED, "ttr_mode_sandwich: core too large"),
        (sandwich(Z=None), INVALID, "ttr_mode_sandwich: null pointer"),
        (sandwich(as_=None), INVALID, "ttr_mode_sandwich: null pointer"),
        (sandwich(Q=A0), INVALID, "ttr_mode_sandwich: Q must not alias an input"),
        (sandwich(Q=A3), INVALID, "ttr_mode_sandwich: Q must not alias an input"),
        (sandwich(as_=(1, R, R * 20)), UNSUPPORTED, "ttr_mode_sandwich: A must be contiguous"),
        (sandwich(wsb=0), WORKSPACE, "ttr_mode_sandwich: workspace 0 < 1280 bytes"),
        (sandwich(dtype=F64, wsb=2559), WORKSPACE, "ttr_mode_sandwich: workspace 2559 < 2560 bytes"),
        (sandwich(ws=None), WORKSPACE, "ttr_mode_sandwich: workspace 1048576 < 1280 bytes"),
    ]
    + [
        (convolve(dtype=7), INVALID, "ttr_core_convolve: bad dtype 7"),
        (convolve(J=0), INVALID, "ttr_core_convolve: bad sizes [2, 5, 3] x [2, 0, 3], K = 8"),
        (convolve(I=1 << 31, K=1), UNSUPPORTED, "ttr_core_convolve: an extent does not fit 32 bits"),
        (convolve(lo=-1), INVALID, "ttr_core_convolve: window (lo = -1, K = 8) outside the full result of 8 entries"),
        (convolve(K=9), INVALID, "ttr_core_convolve: window (lo = 0, K = 9) outside the full result of 8 entries"),
        (convolve(lo=1), INVALID, "ttr_core_convolve: window (lo = 1, K = 8) outside the full result of 8 entries"),
        (convolve(c=None), INVALID, "ttr_core_convolve: null pointer"),
        (convolve(out=A1), INVALID, "ttr_core_convolve: out must not be an input"),
        (convolve(R1=1 << 16, S1=1 << 16), UNSUPPORTED, "ttr_core_convolve: result too large"),
    ]
    + [
        (bad_dtype("ttr_accept_count"), INVALID, "ttr_accept_count: bad dtype 7"),
        (bad_dtype("ttr_accept_expand"), INVALID, "ttr_accept_expand: bad dtype 7"),
        (bad_dtype("ttr_als_normal"), INVALID, "ttr_als_normal: bad dtype 7"),
        (bad_dtype("ttr_spd_solve"), INVALID, "ttr_spd_solve: bad dtype 7"),
        (bad_dtype("ttr_pinv_finish"), INVALID, "ttr_pinv_finish: bad dtype 7"),
        (bad_dtype("ttr_maxvol"), INVALID, "ttr_maxvol: bad dtype 7"),
        (bad_dtype("ttr_maxvol_workspace_bytes"), -1, None),                 # a size query: -1 and no text of its own
        (bad_dtype("ttr_gather_chain"), INVALID, "ttr_gather_chain: bad dtype 7"),
        (bad_dtype("ttr_gather_step"), INVALID, "ttr_gather_step: bad dtype 7"),
        (bad_dtype("ttr_gather_chain_workspace_bytes"), -1, None),
        (bad_dtype("ttr_sparse_gram"), INVALID, "ttr_sparse_gram: bad dtype 7"),
        (bad_dtype("ttr_sparse_gram_parts"), INVALID, "ttr_sparse_gram_parts: bad dtype 7"),
        (bad_dtype("ttr_sparse_gram_workspace_bytes"), INVALID, "ttr_sparse_gram_workspace_bytes: bad dtype 7"),
        (bad_dtype("ttr_sparse_project"), INVALID, "ttr_sparse_project: bad dtype 7"),
        (bad_dtype("ttr_pce_design"), INVALID, "ttr_pce_design: bad dtype 7"),
        (bad_dtype("ttr_pce_predict"), INVALID, "ttr_pce_predict: bad dtype 7"),
        (("ttr_round_tt_workspace_bytes", (7, 3, i64((1, 4, 2, 2, 4, 2, 2, 4, 1)), None, 1, 0)), INVALID, "ttr_round_tt: bad dtype 7"),
    ]
)


def bind(path):
    """the library at `path` with the header's signatures on every entry"""
    from tntorch_amd import _hip

    lib = ctypes.CDLL(path)
    for name, (res, args) in _hip._SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def refusal(lib, call):
    """(status, text) the library answers `call` = (entry, arguments) with"""
    name, args = call
    status = getattr(lib, name)(*args)
    return status, lib.ttr_last_error().decode()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()  # hipcc cross-compiles gfx950 without a GPU
    return bind(g.LIB)


def test_the_table_is_whole():
    assert len(set(name for (name, _), _, _ in CASES)) == 27   # the entries whose checks the shared helpers serve
    assert len(CASES) >= 141


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda k: f"{k}-{CASES[k][0][0]}")
def test_refusal(lib, case):
    call, status, text = CASES[case]
    got_status, got_text = refusal(lib, call)
    assert got_status == status
    if text is not None:
        assert got_text == text

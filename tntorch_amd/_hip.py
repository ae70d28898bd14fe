"""ctypes binding of ``libttround_hip.so`` (the C ABI declared in ``include/ttround_hip.h``).

There is no fallback: a CUDA/HIP tensor reaching the hot path without the built
library raises ``RuntimeError``.  Torch is used here only for device memory
(``torch.empty``) and to obtain the current HIP stream.

The header is the only statement of the ABI: every signature (``_SIGNATURES``) and every constant (``TTR_X`` is ``X`` here)
is parsed from it at import, so a new entry point is declared in the header and gets its wrapper below, nothing else.
"""

from __future__ import annotations

import ctypes
import os
import re
from ctypes import c_char_p, c_double, c_int, c_int64, c_void_p
from typing import Optional, Tuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# TTR_LIB_PATH: load another build of the same library (kernel experiments: several variants side by side)
LIB_PATH = os.environ.get("TTR_LIB_PATH") or os.path.join(_HERE, "libttround_hip.so")

_HEADER = os.path.join(os.path.dirname(_HERE), "include", "ttround_hip.h")
_SCALARS = {"int": c_int, "int64_t": c_int64, "double": c_double}
_POINTEES = ("void", "char", "int", "int32_t", "int64_t", "double")
_C_DECL = re.compile(r"(const\s+)?(\w+)\s*((?:\*\s*(?:const\b\s*)?)*)(?:\w+\s*)?((?:\[\w*\]\s*)*)")


def _ctype(text: str):
    """ctypes type of a C return type or of one parameter (its name is dropped): the scalars of ``_SCALARS``, ``const char*``
    -> c_char_p, every other pointer or array of a ``_POINTEES`` type -> c_void_p; anything else is an error."""
    m = _C_DECL.fullmatch(text.strip())
    if m:
        const, base, stars, dims = m.groups()
        if (stars or dims) and base in _POINTEES:
            return c_char_p if const and base == "char" and stars.strip() == "*" and not dims else c_void_p
        if not (stars or dims or const) and base in _SCALARS:
            return _SCALARS[base]
    raise ValueError(f"include/ttround_hip.h: no ctypes mapping for {text.strip()!r}")


def _parse_header(text: str):
    """({name: (restype, [argtypes])} of every ``ttr_*`` declaration, {name: value} of every ``#define TTR_X <integer>``) of
    the header's text.  Whatever is neither (after comments, other preprocessor lines and the extern "C" braces) is an error."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(TTR_\w+)(.*)$", text, flags=re.M):
        m = re.fullmatch(r"\s+(?:(-?\d+)|\((-?\d+)\))\s*", value)
        if not m or name in defines:
            raise ValueError(f"include/ttround_hip.h: #define {name}{value}: not one integer constant")
        defines[name] = int(m.group(1) or m.group(2))
    code = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    code = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", code, flags=re.S)
    signatures = {}
    for stmt in filter(None, (st.strip() for st in code.split(";"))):
        m = re.fullmatch(r"([^()]+?)\b(ttr_\w+)\s*\(([^()]*)\)", stmt)
        if not m or m.group(2) in signatures:
            raise ValueError(f"include/ttround_hip.h: not a (single) declaration of a ttr_* function: {stmt!r}")
        res, name, params = m.groups()
        signatures[name] = (_ctype(res), [] if params.strip() == "void" else [_ctype(a) for a in params.split(",")])
    return signatures, defines


_lib = None

# name -> (restype, argtypes) of every entry point and TTR_X -> value of every constant: read from the header, which is the
# only statement of the ABI.  Every TTR_X is X here (F32, SCALE_MUL, EIG_RAW, SOLVER_TRIDIAG, ALG_SVD, KNOB_QR_PACK, E_INVALID, ...)
with open(_HEADER) as _f:
    _SIGNATURES, _DEFINES = _parse_header(_f.read())
globals().update({k[len("TTR_"):]: v for k, v in _DEFINES.items()})
PROF_KINDS = tuple(k[len("TTR_PROF_"):].lower() for k in sorted(_DEFINES, key=_DEFINES.get)
                   if k.startswith("TTR_PROF_") and k != "TTR_PROF_NKINDS")
if len(PROF_KINDS) != _DEFINES["TTR_PROF_NKINDS"]:
    raise ValueError(f"include/ttround_hip.h: TTR_PROF_NKINDS = {_DEFINES['TTR_PROF_NKINDS']}, but the kinds are {PROF_KINDS}")

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def available() -> bool:
    return os.path.exists(LIB_PATH)


def lib():
    """Load the shared library (once).  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the HIP kernels are not built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C tntorch_amd/csrc`). "
                "tntorch_amd has no CPU/torch fallback for GPU tensors."
            )
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.ttr_version() != ABI_VERSION:
            raise RuntimeError(
                f"{LIB_PATH} was built for ABI version {L.ttr_version()}, this binding expects {ABI_VERSION} "
                "(include/ttround_hip.h: TTR_ABI_VERSION): rebuild with `python __graft_entry__.py --force`.")
        # A/B measurements without code changes: TTR_KNOBS="6=0,0=1" calls ttr_debug_set_knob(6, 0), (0, 1) once after loading
        for item in filter(None, os.environ.get("TTR_KNOBS", "").split(",")):
            k, v = item.split("=")
            if L.ttr_debug_set_knob(int(k), int(v)) != 0:
                raise ValueError(f"TTR_KNOBS: ttr_debug_set_knob({k}, {v}) rejected: " + L.ttr_last_error().decode(errors="replace"))
        # The eps-mode rank rule sees null directions at LAPACK's noise floor (header: TTR_KNOB_RANK_NOISE_FLOOR = 1, the library's
        # default since round 6: the reference's ranks).  TTR_STRICT_RANKS=0 switches the floor off: exact zeros are cut
        # (INTEGRATION.md "Ranks of rank-deficient trains")
        if os.environ.get("TTR_STRICT_RANKS", "1") == "0":
            L.ttr_debug_set_knob(KNOB_RANK_NOISE_FLOOR, 0)
        # TTR_ORTH_SPLIT=<batch size>: ttr_orth_fixup's three-launch rounds from that batch size on (header: TTR_KNOB_ORTH_SPLIT)
        if os.environ.get("TTR_ORTH_SPLIT", "") != "":
            L.ttr_debug_set_knob(KNOB_ORTH_SPLIT, int(os.environ["TTR_ORTH_SPLIT"]))
        _lib = L
    return _lib


def _check(code: int, what: str):
    if code != 0:
        msg = lib().ttr_last_error().decode(errors="replace")
        if code == E_UNSUPPORTED:
            raise NotImplementedError(f"{what}: {msg}")
        if code == E_INVALID:
            raise ValueError(f"{what}: {msg}")
        raise RuntimeError(f"{what} failed ({code}): {msg}")


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return F32
    if dt == torch.float64:
        return F64
    raise TypeError(f"tntorch_amd HIP path supports float32/float64 tensors only, got {dt}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _call(name: str, *args):
    """Launch the entry point ``name`` (one whose last parameter is ``void* stream``) on the current stream and check its status."""
    _check(getattr(lib(), name)(*args, _stream()), name)


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return t.data_ptr() if t is not None else None


def _workspace(nbytes: int, device, floor: int = 0) -> Optional[torch.Tensor]:
    """uint8 scratch of max(nbytes, floor) bytes, or None (the library then receives a null pointer) when that is 0."""
    nbytes = max(nbytes, floor)
    return torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes > 0 else None


def _first_cuda_tensor(args, kwargs):
    for a in args:
        if isinstance(a, torch.Tensor) and a.is_cuda:
            return a
        if isinstance(a, QrFactors):
            return a.ws
    for a in kwargs.values():
        if isinstance(a, torch.Tensor) and a.is_cuda:
            return a
    return None


def _on_device(fn):
    """Run a binding with the device of its first device operand current: workspaces / results are allocated there
    and ``_stream()`` is that device's current stream (a tensor on cuda:1 while cuda:0 is current would otherwise be
    processed on cuda:0's stream -- a cross-device launch, unordered against torch's work on cuda:1)."""
    import functools

    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        t = _first_cuda_tensor(args, kwargs)
        if t is None or t.device.index is None or t.device.index == torch.cuda.current_device():
            return fn(*args, **kwargs)
        with torch.cuda.device(t.device):
            return fn(*args, **kwargs)

    return wrapped


def _mat(t: torch.Tensor) -> Tuple[torch.Tensor, int, int]:
    """Return (tensor, ld, batch_stride) of a [B, r, c] tensor whose rows are contiguous."""
    assert t.dim() == 3 and t.is_cuda
    B, r, c = t.shape
    ok = (c == 1 or t.stride(2) == 1) and (r == 1 or t.stride(1) >= max(c, 1)) and (B == 1 or t.stride(0) >= 0)
    if not ok:
        t = t.contiguous()
    ld = t.stride(1) if r > 1 else max(c, 1)
    bs = t.stride(0) if B > 1 else r * ld
    return t, int(ld), int(bs)


def max_qr_cols(dt: torch.dtype) -> int:
    return lib().ttr_qr_max_cols(dtype_code(dt))


def max_eigh_n(dt: torch.dtype = torch.float32) -> int:
    return lib().ttr_eigh_max_n(dtype_code(dt))


# ----------------------------------------------------------------------------------------------
@_on_device
def gemm(
    A: torch.Tensor,
    B: torch.Tensor,
    transA: bool = False,
    transB: bool = False,
    rowscale: Optional[torch.Tensor] = None,
    rowscale_mode: int = SCALE_NONE,
    colscale: Optional[torch.Tensor] = None,
    colscale_mode: int = SCALE_NONE,
    out: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """C[b] = scale(op(A[b]) @ op(B[b])) for [batch, ., .] tensors; returns a fresh tensor (or ``out``, a
    contiguous [batch, M, N] tensor -- e.g. a batch slice of a larger result -- that is overwritten)."""
    L = lib()
    dt = dtype_code(A.dtype)
    assert A.dtype == B.dtype and A.shape[0] == B.shape[0]
    A, lda, sA = _mat(A)
    B, ldb, sB = _mat(B)
    batch = A.shape[0]
    M, K = (A.shape[2], A.shape[1]) if transA else (A.shape[1], A.shape[2])
    K2, N = (B.shape[2], B.shape[1]) if transB else (B.shape[1], B.shape[2])
    if K != K2:
        raise ValueError(f"gemm: inner dimensions differ ({K} vs {K2})")
    if out is not None:
        assert tuple(out.shape) == (batch, M, N) and out.is_contiguous() and out.dtype == A.dtype
        C = out
    else:
        C = torch.empty((batch, M, N), dtype=A.dtype, device=A.device)
    if M == 0 or N == 0 or batch == 0:
        return C
    rs_ptr, rs_stride = None, 0
    if rowscale is not None:
        rowscale = rowscale.contiguous()
        rs_ptr, rs_stride = rowscale.data_ptr(), rowscale.shape[-1]
    cs_ptr, cs_stride = None, 0
    if colscale is not None:
        colscale = colscale.contiguous()
        cs_ptr, cs_stride = colscale.data_ptr(), colscale.shape[-1]
    wsb = L.ttr_gemm_workspace_bytes(dt, M, N, K, batch)
    ws = _workspace(wsb, A.device)
    _call("ttr_gemm", dt, int(transA), int(transB), M, N, K,
          A.data_ptr(), lda, sA, B.data_ptr(), ldb, sB, C.data_ptr(), N, M * N,
          rs_ptr, rs_stride, rowscale_mode if rowscale is not None else SCALE_NONE,
          cs_ptr, cs_stride, colscale_mode if colscale is not None else SCALE_NONE,
          batch, _ptr(ws), wsb)
    return C


@_on_device
def gemm_axpby(A: torch.Tensor, B: torch.Tensor, C: torch.Tensor, alpha: float, beta: float,
               transA: bool = False, transB: bool = False) -> torch.Tensor:
    """In place: C[b] <- beta * C[b] + alpha * op(A[b]) @ op(B[b]); C must be contiguous [batch, M, N]."""
    L = lib()
    dt = dtype_code(A.dtype)
    assert A.dtype == B.dtype == C.dtype and A.shape[0] == B.shape[0] == C.shape[0]
    assert C.is_contiguous()
    A, lda, sA = _mat(A)
    B, ldb, sB = _mat(B)
    batch = A.shape[0]
    M, K = (A.shape[2], A.shape[1]) if transA else (A.shape[1], A.shape[2])
    K2, N = (B.shape[2], B.shape[1]) if transB else (B.shape[1], B.shape[2])
    if K != K2 or tuple(C.shape) != (batch, M, N):
        raise ValueError(f"gemm_axpby: shapes do not match ({K} vs {K2}, C {tuple(C.shape)})")
    if M == 0 or N == 0 or batch == 0:
        return C
    wsb = L.ttr_gemm_workspace_bytes(dt, M, N, K, batch)
    ws = _workspace(wsb, A.device)
    _call("ttr_gemm_axpby", dt, int(transA), int(transB), M, N, K,
          A.data_ptr(), lda, sA, B.data_ptr(), ldb, sB, C.data_ptr(), N, M * N,
          float(alpha), float(beta), batch, _ptr(ws), wsb)
    return C


@_on_device
def qr(A: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Reduced Householder QR of [batch, m, n] -> Q [batch, m, k], R [batch, k, n]."""
    L = lib()
    dt = dtype_code(A.dtype)
    A, lda, sA = _mat(A)
    batch, m, n = A.shape
    k = min(m, n)
    Q = torch.empty((batch, m, k), dtype=A.dtype, device=A.device)
    R = torch.empty((batch, k, n), dtype=A.dtype, device=A.device)
    if batch == 0:
        return Q, R
    wsb = L.ttr_qr_workspace_bytes(dt, m, n, batch)
    ws = _workspace(wsb, A.device, 16)
    _call("ttr_qr", dt, m, n, batch, A.data_ptr(), lda, sA, Q.data_ptr(), k, m * k, R.data_ptr(), n, k * n, ws.data_ptr(), wsb)
    return Q, R


@_on_device
def qr_t(At: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """QR of the TRANSPOSE of ``At`` [batch, n, m] without transposing it: returns (Qt [batch, k, m] = Q^T, R [batch, k, n])
    (ttr_qr_t: the kernels address the operand and the result through strides)."""
    L = lib()
    dt = dtype_code(At.dtype)
    At, ldat, sAt = _mat(At)
    batch, n, m = At.shape
    k = min(m, n)
    Qt = torch.empty((batch, k, m), dtype=At.dtype, device=At.device)
    R = torch.empty((batch, k, n), dtype=At.dtype, device=At.device)
    if batch == 0:
        return Qt, R
    wsb = L.ttr_qr_workspace_bytes(dt, m, n, batch)
    ws = _workspace(wsb, At.device, 16)
    _call("ttr_qr_t", dt, m, n, batch, At.data_ptr(), ldat, sAt, Qt.data_ptr(), m, k * m, R.data_ptr(), n, k * n,
          ws.data_ptr(), wsb)
    return Qt, R


class QrFactors:
    """Handle on a factored batch (reflectors + T factors live in ``ws``) for later ``qr_apply`` calls."""

    __slots__ = ("ws", "wsb", "m", "n", "batch", "dtype", "R", "pushed", "rows32")

    def __init__(self, ws, wsb, m, n, batch, dtype, R, pushed=None, rows32=None):
        self.ws, self.wsb, self.m, self.n, self.batch, self.dtype, self.R = ws, wsb, m, n, batch, dtype, R
        self.pushed = pushed  # (k, I) when the factorisation came from qr_factor_pushed
        # int32 [batch] view into ``ws`` (pushed factorisations): != 0 for items whose level-0 blocks packed their rows -- rows
        # kk >= 32 of what qr_apply produces from this handle are exactly zero (ttr_rowgram / ttr_project: ``rows32``)
        self.rows32 = rows32

    @property
    def k(self):
        return min(self.m, self.n)


@_on_device
def qr_factor(A: torch.Tensor, expo_acc: Optional[torch.Tensor] = None) -> QrFactors:
    """Factor [batch, m, n]; returns a handle holding R [batch, k, n] and the implicit Q.

    ``expo_acc`` (fp32; device int32 [batch]): R comes back as R 2^-e, e the exponent of the top block's largest entry, and e is
    added to expo_acc[b] -- the sweep's per-core power-of-two normalisation without a launch of its own (ttr_qr_factor_expo)."""
    L = lib()
    dt = dtype_code(A.dtype)
    A, lda, sA = _mat(A)
    batch, m, n = A.shape
    k = min(m, n)
    R = torch.empty((batch, k, n), dtype=A.dtype, device=A.device)
    wsb = L.ttr_qr_workspace_bytes(dt, m, n, max(batch, 1))
    ws = _workspace(wsb, A.device, 16)
    if batch > 0 and expo_acc is not None:
        assert expo_acc.dtype == torch.int32 and expo_acc.numel() == batch and expo_acc.is_contiguous()
        _call("ttr_qr_factor_expo", dt, m, n, batch, A.data_ptr(), lda, sA, R.data_ptr(), n, k * n, ws.data_ptr(), wsb,
              expo_acc.data_ptr())
    elif batch > 0:
        _call("ttr_qr_factor", dt, m, n, batch, A.data_ptr(), lda, sA, R.data_ptr(), n, k * n, ws.data_ptr(), wsb)
    return QrFactors(ws, wsb, m, n, batch, A.dtype, R)


def pushed_supported(k: int, Rin: int, I: int, n: int, dt: torch.dtype) -> bool:
    return k <= 64 and Rin <= 64 and n <= max_qr_cols(dt) and k * I >= n


@_on_device
def qr_factor_pushed(Rm: torch.Tensor, core4: torch.Tensor, expo_acc: Optional[torch.Tensor] = None) -> QrFactors:
    """Factor the left unfolding of ``Rm @ core`` (Rm [batch, k, Rin], core [batch, Rin, I, n]) without forming it.
    ``expo_acc``: as for ``qr_factor`` (ttr_qr_factor_pushed_expo)."""
    L = lib()
    dt = dtype_code(core4.dtype)
    Rm, ldrm, sRm = _mat(Rm)
    core4 = core4.contiguous()
    batch, Rin, I, n = core4.shape
    k = Rm.shape[1]
    assert Rm.shape[2] == Rin and Rm.shape[0] == batch
    kq = min(k * I, n)
    R = torch.empty((batch, kq, n), dtype=core4.dtype, device=core4.device)
    wsb = L.ttr_qr_pushed_workspace_bytes(dt, I, n, max(batch, 1))
    ws = _workspace(wsb, core4.device, 16)
    if batch > 0 and expo_acc is not None:
        assert expo_acc.dtype == torch.int32 and expo_acc.numel() == batch and expo_acc.is_contiguous()
        _call("ttr_qr_factor_pushed_expo", dt, k, Rin, I, n, batch, Rm.data_ptr(), ldrm, sRm, core4.data_ptr(), Rin * I * n,
              R.data_ptr(), n, kq * n, ws.data_ptr(), wsb, expo_acc.data_ptr())
    elif batch > 0:
        _call("ttr_qr_factor_pushed", dt, k, Rin, I, n, batch, Rm.data_ptr(), ldrm, sRm, core4.data_ptr(), Rin * I * n,
              R.data_ptr(), n, kq * n, ws.data_ptr(), wsb)
    flags = None
    if batch > 0 and k == 64:
        off = int(L.ttr_qr_pushed_flag_offset(dt, I, n, batch))
        if off >= 0:
            flags = ws[off:off + 4 * batch].view(torch.int32)
    return QrFactors(ws, wsb, k * I, n, batch, core4.dtype, R, pushed=(k, I), rows32=flags)


@_on_device
def qr_factor_pushed_sum(Rm: torch.Tensor, a4: torch.Tensor, b4: torch.Tensor) -> QrFactors:
    """Factor the left unfolding of ``Rm @ blockdiag(a, b)`` (Rm [batch, k, ra + rb], a [batch, ra, I, ca],
    b [batch, rb, I, cb]) without forming the block-diagonal core of the TT sum (ttr_qr_factor_pushed_sum)."""
    L = lib()
    dt = dtype_code(a4.dtype)
    Rm, ldrm, sRm = _mat(Rm)
    a4, b4 = a4.contiguous(), b4.contiguous()
    batch, ra, I, ca = a4.shape
    _, rb, _, cb = b4.shape
    k, n = Rm.shape[1], ca + cb
    assert Rm.shape[2] == ra + rb and Rm.shape[0] == batch and b4.shape[0] == batch and b4.shape[2] == I
    kq = min(k * I, n)
    R = torch.empty((batch, kq, n), dtype=a4.dtype, device=a4.device)
    wsb = L.ttr_qr_pushed_workspace_bytes(dt, I, n, max(batch, 1))
    ws = _workspace(wsb, a4.device, 16)
    if batch > 0:
        _call("ttr_qr_factor_pushed_sum", dt, k, I, batch, Rm.data_ptr(), ldrm, sRm, a4.data_ptr(), ra, ca, ra * I * ca,
              b4.data_ptr(), rb, cb, rb * I * cb, R.data_ptr(), n, kq * n, ws.data_ptr(), wsb)
    return QrFactors(ws, wsb, k * I, n, batch, a4.dtype, R, pushed=(k, I))


@_on_device
def qr_apply(f: QrFactors, C: Optional[torch.Tensor] = None, kcols: Optional[int] = None,
             out: Optional[torch.Tensor] = None, want_gram: bool = False, skip_zero_rows: bool = False):
    """Out [batch, m, kcols] = Q @ C  (C: [batch, k, kcols]; None -> first ``kcols`` columns of Q).
    ``out``: optional contiguous destination (e.g. a batch slice of a larger result).
    ``want_gram``: return ``(Out, G)``; G = split partials [batch, parts, k, k] of the row Gram matrix of Out's
    k x (I kcols) right unfolding, accumulated by the apply kernel itself (ttr_qr_apply_pushed_gram), or None when
    the shape is not covered (the caller then runs ``rowgram``)."""
    L = lib()
    dt = dtype_code(f.dtype)
    if C is not None:
        C, ldc, sC = _mat(C)
        assert C.shape[0] == f.batch and C.shape[1] == f.k
        kcols = C.shape[2]
        cptr = C.data_ptr()
    else:
        kcols = f.k if kcols is None else kcols
        ldc, sC, cptr = 0, 0, None
    if out is not None:
        assert tuple(out.shape) == (f.batch, f.m, kcols) and out.is_contiguous() and out.dtype == f.dtype
        Out = out
    else:
        Out = torch.empty((f.batch, f.m, kcols), dtype=f.dtype, device=f.ws.device)
    G = None
    if f.batch == 0:
        return (Out, G) if want_gram else Out
    if f.pushed is not None:
        k, I = f.pushed
        parts = int(L.ttr_qr_apply_pushed_gram_parts(dt, k, I, f.n, kcols)) if want_gram else 0
        if parts > 0:
            G = torch.empty((f.batch, parts, k, k), dtype=f.dtype, device=f.ws.device)
            _call("ttr_qr_apply_pushed_gram", dt, k, I, f.n, f.batch, f.ws.data_ptr(), f.wsb, cptr, ldc, sC, kcols,
                  Out.data_ptr(), kcols, f.m * kcols, G.data_ptr())
        else:
            # skip_zero_rows: the rows kk >= 32 of packed items (f.rows32) stay unwritten -- only for results that are read
            # through the rows32-aware kernels (rowgram / rotgram / project)
            _call("ttr_qr_apply_pushed", dt, k, I, f.n, f.batch, f.ws.data_ptr(), f.wsb, cptr, ldc, sC, kcols, Out.data_ptr(),
                  kcols, f.m * kcols, int(bool(skip_zero_rows and f.rows32 is not None)))
        return (Out, G) if want_gram else Out
    _call("ttr_qr_apply", dt, f.m, f.n, f.batch, f.ws.data_ptr(), f.wsb, cptr, ldc, sC, kcols, Out.data_ptr(), kcols, f.m * kcols)
    return (Out, G) if want_gram else Out


@_on_device
def eigh_trunc(
    G: torch.Tensor, eig_mode: int, use_delta: bool, delta2: float, rmax: int, abs_floor: int = 1,
    sweeps: Optional[torch.Tensor] = None, delta2_dev: Optional[torch.Tensor] = None,
    skip_items: Optional[torch.Tensor] = None, sigma_in: Optional[torch.Tensor] = None, skip_lean: bool = False,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Eigen-decomposition of symmetric [batch, n, n] + rank rule.  Returns V (columns sorted by
    decreasing sigma), sigma [batch, n], info [batch] int32 (rank, or 0 for the zero guard).
    ``G`` may also be [batch, parts, n, n] (contiguous): split-K partials of a Gram kernel, summed on load.
    ``skip_lean``: ttr_eigh_trunc_pass -- V of the ``skip_items`` is left unwritten (the caller hands the same flags to
    ``project(flat=...)``, which does not read it)."""
    L = lib()
    dt = dtype_code(G.dtype)
    gparts, sGp = 1, 0
    if G.dim() == 4:
        G = G.contiguous()
        batch, gparts, n, _ = G.shape
        ldg, sG, sGp = n, gparts * n * n, n * n
    else:
        G, ldg, sG = _mat(G)
        batch, n, _ = G.shape
    V = torch.empty((batch, n, n), dtype=G.dtype, device=G.device)
    sigma = torch.empty((batch, n), dtype=G.dtype, device=G.device)
    info = torch.empty((batch,), dtype=torch.int32, device=G.device)
    if batch == 0:
        return V, sigma, info
    wsb = L.ttr_eigh_workspace_bytes(dt, n, batch)
    ws = _workspace(wsb, G.device)
    rmax = int(min(max(int(rmax), 1), 2**31 - 1))
    _call("ttr_eigh_trunc_pass" if skip_lean else "ttr_eigh_trunc", dt, n, batch, G.data_ptr(), ldg, sG, gparts, sGp, V.data_ptr(), n, n * n, sigma.data_ptr(), n,
          info.data_ptr(), eig_mode, int(bool(use_delta)), float(delta2), _ptr(delta2_dev), rmax, int(abs_floor),
          _ptr(sweeps), _ptr(skip_items), _ptr(sigma_in), sigma_in.shape[-1] if sigma_in is not None else 0, _ptr(ws), wsb)
    return V, sigma, info


def eigh_top_ok(n: int, r: int) -> bool:
    return bool(lib().ttr_eigh_top_ok(int(n), int(r)))


@_on_device
def eigh_top(G: torch.Tensor, r: int, thr: float, need_all: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Pass 1 of a batch-mode bond: symmetric [batch, n, n] (or split partials [batch, parts, n, n]), 40 <= n <= 64, rank cap
    r <= 32 (ttr_eigh_top).  Returns (V, sigma, info, flat): items with flat[b] = 1 carry their r largest eigenpairs (V[b][:, :r],
    sigma[b][:r], zeros beyond), the others the full decomposition of ``eigh_trunc(G, EIG_RAW, ..., abs_floor=SOLVER_TRIDIAG)``
    (flat[b] = 2 when its kept sigma pass ``spectrum_flat``'s batch-mode test, else 0).  ``need_all``: eps mode -- the top-r path only
    takes items whose every eigenpair it computes (zero-tail items under a cap >= 32); sigma / V are complete for every item."""
    dt = dtype_code(G.dtype)
    gparts, sGp = 1, 0
    if G.dim() == 4:
        G = G.contiguous()
        batch, gparts, n, _ = G.shape
        ldg, sG, sGp = n, gparts * n * n, n * n
    else:
        G, ldg, sG = _mat(G)
        batch, n, _ = G.shape
    V = torch.empty((batch, n, n), dtype=G.dtype, device=G.device)
    sigma = torch.empty((batch, n), dtype=G.dtype, device=G.device)
    info = torch.empty((batch,), dtype=torch.int32, device=G.device)
    flat = torch.empty((batch,), dtype=torch.int32, device=G.device)
    if batch:
        _call("ttr_eigh_top", dt, n, batch, G.data_ptr(), ldg, sG, gparts, sGp, V.data_ptr(), n, n * n, sigma.data_ptr(), n,
              info.data_ptr(), int(r), float(thr), flat.data_ptr(), int(bool(need_all)))
    return V, sigma, info, flat


@_on_device
def eigh_topk(G: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The k largest eigenpairs of symmetric [batch, n, n] (64 < n <= ttr_eigsel_max_n(), k <= 64): tridiagonalisation,
    multisection + twisted factorisation on the tridiagonal matrix, TSQR of the k vectors, back-transformation (ttr_tridiag,
    ttr_tri_eigsel, ttr_qr, ttr_tridiag_back).  Returns (X [batch, n, k] orthonormal, lam [batch, k] descending,
    rmin [batch] = the smallest |R_jj| of the orthonormalisation: well below 1 when two of the k vectors nearly coincided --
    clustered or multiple eigenvalues, which this solver does not resolve; the caller decides).
    The size range: include/ttround_hip.h words the family as "symmetric matrices with 64 < n <= ttr_eigsel_max_n()" -- that is
    where it is used and tuned (below it the single-workgroup eigensolvers are faster).  The contract of the three entry points
    is wider: each accepts 2 <= n <= ttr_eigsel_max_n() (k <= min(64, n) for ttr_tri_eigsel) and refuses everything else with
    TTR_E_UNSUPPORTED; this wrapper adds no check of its own (tests/test_eigsel_kernels_gpu.py drives the entry points
    from n = 2)."""
    L = lib()
    dt = dtype_code(G.dtype)
    batch, n, _ = G.shape
    A = G.contiguous().clone()  # destroyed by the reduction
    d = torch.empty((batch, n), dtype=G.dtype, device=G.device)
    e = torch.empty_like(d)
    tau = torch.empty_like(d)
    lam = torch.empty((batch, k), dtype=G.dtype, device=G.device)
    Z = torch.empty((batch, n, k), dtype=G.dtype, device=G.device)
    if batch == 0:
        return Z, lam, torch.empty((0,), dtype=G.dtype, device=G.device)
    wsb = L.ttr_tridiag_workspace_bytes(dt, n, batch)
    ws = torch.empty(wsb, dtype=torch.uint8, device=G.device)
    _call("ttr_tridiag", dt, n, batch, A.data_ptr(), n, n * n, d.data_ptr(), e.data_ptr(), tau.data_ptr(), ws.data_ptr(), wsb)
    sb = L.ttr_eigsel_scratch_bytes(dt, n, batch)
    scratch = torch.empty(sb, dtype=torch.uint8, device=G.device)
    _call("ttr_tri_eigsel", dt, n, batch, int(k), d.data_ptr(), e.data_ptr(), lam.data_ptr(), Z.data_ptr(),
          scratch.data_ptr(), sb)
    Zq, R = qr(Z)
    rmin = torch.diagonal(R, dim1=1, dim2=2).abs().amin(dim=1)
    Zq = Zq.contiguous()
    _call("ttr_tridiag_back", dt, n, batch, int(k), A.data_ptr(), n, n * n, tau.data_ptr(), Zq.data_ptr())
    return Zq, lam, rmin


_BJ_TABLES: dict = {}


def bj_pair_tables(nbk: int, device) -> torch.Tensor:
    """Round-robin tournament over an even number of blocks: int32 [nbk - 1, nbk / 2, 2] on the device (cached)."""
    key = (nbk, str(device))
    if key not in _BJ_TABLES:
        assert nbk % 2 == 0 and nbk >= 2
        circle = list(range(nbk))
        rounds = []
        for _ in range(nbk - 1):
            rounds.append([[circle[i], circle[-1 - i]] for i in range(nbk // 2)])
            circle = [circle[0], circle[-1]] + circle[1:-1]
        _BJ_TABLES[key] = torch.tensor(rounds, dtype=torch.int32).to(device)
    return _BJ_TABLES[key]


@_on_device
def bj_sweeps(G: torch.Tensor, V: torch.Tensor, b: int, relative: bool, tol: float, max_sweeps: int) -> torch.Tensor:
    """Block-Jacobi sweeps on G [B, n, n] / V [B, n, n] IN PLACE (ttr_bj_solve / ttr_bj_apply / ttr_bj_control).  The
    convergence word is read back once per tranche of 8 sweeps (control flow only: the launches of a converged driver return at
    their first instruction, but each still costs a launch).  Returns the device control block (int32 [4]: converged, -, sweeps
    performed, -) for diagnostics."""
    L = lib()
    dt = dtype_code(G.dtype)
    Bt, n, _ = G.shape
    nbk = n // b
    assert n == nbk * b and nbk % 2 == 0 and G.is_contiguous() and V.is_contiguous()
    npairs, w = nbk // 2, 2 * b
    tabs = bj_pair_tables(nbk, G.device)
    ctrl = torch.zeros(4, dtype=torch.int32, device=G.device)
    state = torch.zeros(Bt + 1, dtype=torch.float64, device=G.device)
    state[Bt:].fill_(-1.0)
    gn = norm(G.reshape(Bt, -1)) if not relative else None
    W = torch.empty((Bt * npairs, w, w), dtype=G.dtype, device=G.device)
    scratch = _workspace(int(L.ttr_bj_scratch_bytes(dt, b, npairs, Bt)), G.device, 16)
    st = _stream()
    rounds = nbk - 1
    tranche = 8   # sweeps enqueued before the convergence word is looked at (one readback: control flow only).  Convergence
                  # typically comes after 6 .. 10 sweeps; the launches of the remaining sweeps of max_sweeps would return at their
                  # first instruction, but each still costs a launch (n = 1024, b = 32: 63 launches per sweep)
    for sweep in range(max_sweeps):
        if sweep > 0 and sweep % tranche == 0 and int(ctrl[0].item()) != 0:
            break
        for r in range(rounds):
            tab = tabs[r].data_ptr()
            _check(L.ttr_bj_solve(dt, b, npairs, Bt, G.data_ptr(), n, n * n, tab, W.data_ptr(), scratch.data_ptr(),
                                  ctrl.data_ptr(), st), "ttr_bj_solve")
            off = state.data_ptr() if (not relative and r == rounds - 1) else None
            _check(L.ttr_bj_apply(dt, b, npairs, Bt, G.data_ptr(), n, n * n, V.data_ptr(), n, n * n, tab, W.data_ptr(),
                                  ctrl.data_ptr(), off, st), "ttr_bj_apply")
        _check(L.ttr_bj_control(dt, Bt, ctrl.data_ptr(), state.data_ptr(), _ptr(gn), int(relative), float(tol), st),
               "ttr_bj_control")
    return ctrl


@_on_device
def norm(x: torch.Tensor) -> torch.Tensor:
    """Frobenius norm per batch item of a [batch, ...] tensor -> [batch]."""
    dt = dtype_code(x.dtype)
    x = x.contiguous()
    batch = x.shape[0]
    count = x[0].numel() if batch > 0 else 0
    out = torch.empty((batch,), dtype=x.dtype, device=x.device)
    if batch == 0:
        return out
    if count >= (1 << 20) and batch < 512:
        # ttr_norm runs one workgroup per batch item: split long items into k chunks (norm of the chunk
        # norms is exact: the second stage squares and sums in double) so that the whole chip streams
        k = 4096
        while k > 1 and count % k:
            k //= 2
        if k > 1:
            part = norm(x.reshape(batch * k, count // k))
            return norm(part.reshape(batch, k))
    _call("ttr_norm", dt, count, batch, x.data_ptr(), count, out.data_ptr())
    return out


@_on_device
def scale_cols(X: torch.Tensor, s: torch.Tensor, mode: int) -> torch.Tensor:
    """out[b, i, j] = X[b, i, j] * s[b, j] (SCALE_MUL) or / s[b, j] (SCALE_DIV)."""
    dt = dtype_code(X.dtype)
    X, ldx, sX = _mat(X)
    s = s.contiguous()
    batch, rows, cols = X.shape
    out = torch.empty((batch, rows, cols), dtype=X.dtype, device=X.device)
    if out.numel() == 0:
        return out
    _call("ttr_scale_cols", dt, rows, cols, batch, X.data_ptr(), ldx, sX, s.data_ptr(), s.shape[-1], mode,
          out.data_ptr(), cols, rows * cols)
    return out


@_on_device
def mask_cols(X: torch.Tensor, keep: torch.Tensor) -> torch.Tensor:
    """In place: X[b, :, j] = 0 for j >= keep[b] (keep: int32 [batch] on the device)."""
    X3, ldx, sX = _mat(X)
    assert X3.data_ptr() == X.data_ptr() and keep.dtype == torch.int32 and keep.shape[0] == X.shape[0]
    _call("ttr_mask_cols", dtype_code(X.dtype), X.shape[1], X.shape[2], X.shape[0], X.data_ptr(), ldx, sX, keep.data_ptr())
    return X


def sweep_fused_ok(M: torch.Tensor) -> bool:
    """The fused row-Gram / rotate-Gram / projection kernels hold up to 64 rows."""
    return M.shape[1] <= 64


@_on_device
def spectrum_flat(sigma: torch.Tensor, keep: int, thr: float, use_delta: bool = False, delta2: float = 0.0,
                  delta2_dev: Optional[torch.Tensor] = None, rows32: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 [batch]: 1 where sigma[b, r - 1] >= thr * sigma[b, 0] > 0 (sigma [batch, n] sorted decreasing), r = keep, or with
    ``use_delta`` the rank the tail-energy rule selects from these sigma provided that decision is robust (ttr_spectrum_flat)."""
    sigma = sigma.contiguous()
    batch, n = sigma.shape
    flat = torch.empty((batch,), dtype=torch.int32, device=sigma.device)
    if batch:
        _call("ttr_spectrum_flat", dtype_code(sigma.dtype), n, batch, sigma.data_ptr(), n, int(keep), float(thr),
              int(bool(use_delta)), float(delta2), _ptr(delta2_dev), flat.data_ptr(), _ptr(rows32))
    return flat


@_on_device
def rowgram(M: torch.Tensor, V1: Optional[torch.Tensor] = None, skip: Optional[torch.Tensor] = None,
            rows32: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Split-K partials [batch, parts, R, R] of M M^T (V1 None) or of (V1^T M)(V1^T M)^T for M [batch, R, n], R <= 64
    (ttr_rowgram / ttr_rotgram); ``eigh_trunc`` sums the parts on load."""
    L = lib()
    dt = dtype_code(M.dtype)
    M, ldm, sM = _mat(M)
    batch, R, n = M.shape
    parts = int(L.ttr_sweep_gram_parts(n, max(batch, 1)))
    G = torch.empty((batch, parts, R, R), dtype=M.dtype, device=M.device)
    if batch == 0:
        return G
    if V1 is None:
        _call("ttr_rowgram", dt, R, n, batch, M.data_ptr(), ldm, sM, G.data_ptr(), parts, _ptr(rows32))
    else:
        V1, ldv, sV = _mat(V1)
        assert V1.shape == (batch, R, R)
        _call("ttr_rotgram", dt, R, n, batch, M.data_ptr(), ldm, sM, V1.data_ptr(), ldv, sV, G.data_ptr(), parts, _ptr(skip),
              _ptr(rows32))
    return G


@_on_device
def project(M: torch.Tensor, V1: Optional[torch.Tensor], V2: torch.Tensor, sigma: Optional[torch.Tensor], ro: int,
            scale_right: bool, out: Optional[torch.Tensor] = None, want_left: bool = True,
            rows32: Optional[torch.Tensor] = None, flat: Optional[torch.Tensor] = None,
            sigma1: Optional[torch.Tensor] = None):
    """right [batch, ro, n] = diag(1/sigma) U^T M and left [batch, R, ro] = U diag(sigma) with U = V1 V2[:, :ro]
    (ttr_project_flat; ``scale_right=False``: right = U^T M, left = U).  ``out``: optional contiguous destination of right.
    ``flat`` / ``sigma1``: the pass-through flags of the two-pass truncation and pass 1's sigma -- flagged items take
    U = V1[:, :ro] and their scales from ``sigma1``; their V2 and sigma are not read."""
    dt = dtype_code(M.dtype)
    M, ldm, sM = _mat(M)
    batch, R, n = M.shape
    V2, ldv2, sV2 = _mat(V2)
    v1p, ldv1, sV1 = None, 0, 0
    if V1 is not None:
        V1, ldv1, sV1 = _mat(V1)
        v1p = V1.data_ptr()
    if out is not None:
        assert tuple(out.shape) == (batch, ro, n) and out.is_contiguous() and out.dtype == M.dtype
        right = out
    else:
        right = torch.empty((batch, ro, n), dtype=M.dtype, device=M.device)
    left = torch.empty((batch, R, ro), dtype=M.dtype, device=M.device) if want_left else None
    if batch == 0:
        return right, left
    sp, ss = None, 0
    if sigma is not None:
        sigma = sigma.contiguous()
        sp, ss = sigma.data_ptr(), sigma.shape[-1]
    s1p, s1s = None, 0
    if flat is not None:
        sigma1 = sigma1.contiguous()
        s1p, s1s = sigma1.data_ptr(), sigma1.shape[-1]
    _call("ttr_project_flat", dt, R, n, ro, batch, M.data_ptr(), ldm, sM, v1p, ldv1, sV1, V2.data_ptr(), ldv2, sV2, sp, ss,
          int(bool(scale_right)), right.data_ptr(), n, ro * n, _ptr(left), ro, R * ro, _ptr(rows32), _ptr(flat), s1p, s1s)
    return right, left


def colsweep_fused_ok(M: torch.Tensor) -> bool:
    """The fused tall-matrix kernels (column Gram / rotated Gram / projection) hold up to 64 columns."""
    return M.shape[2] <= 64


@_on_device
def colgram(M: torch.Tensor, V1: Optional[torch.Tensor] = None, skip: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[batch, n, n] = M^T M (V1 None) or (M V1)^T (M V1) for a tall M [batch, rows, n], n <= 64 (ttr_colgram)."""
    L = lib()
    dt = dtype_code(M.dtype)
    M, ldm, sM = _mat(M)
    batch, rows, n = M.shape
    G = torch.empty((batch, n, n), dtype=M.dtype, device=M.device)
    if batch == 0:
        return G
    wsb = L.ttr_colgram_workspace_bytes(dt, rows, n, batch)
    ws = _workspace(wsb, M.device)
    v1p, ldv, sV = None, 0, 0
    if V1 is not None:
        V1, ldv, sV = _mat(V1)
        assert V1.shape == (batch, n, n)
        v1p = V1.data_ptr()
    _call("ttr_colgram", dt, rows, n, batch, M.data_ptr(), ldm, sM, v1p, ldv, sV, G.data_ptr(), _ptr(ws), wsb, _ptr(skip))
    return G


@_on_device
def colproject(M: torch.Tensor, V1: Optional[torch.Tensor], V2: torch.Tensor, sigma: Optional[torch.Tensor], ro: int,
               left_ortho: bool, left_out: Optional[torch.Tensor] = None):
    """left [batch, rows, ro] = M U [/ sigma], right [batch, ro, n] = [sigma] U^T with U = V1 V2[:, :ro] (ttr_colproject).
    ``left_out``: optional contiguous [batch, rows, ro] destination of ``left`` (may lie in M's own storage BELOW the rows this
    call reads: the in-place first step of a config-scale dense TT-SVD, ``_hipops._colproject_inplace``)."""
    dt = dtype_code(M.dtype)
    M, ldm, sM = _mat(M)
    batch, rows, n = M.shape
    V2, ldv2, sV2 = _mat(V2)
    v1p, ldv1, sV1 = None, 0, 0
    if V1 is not None and rows >= 4096:
        # tall inputs: U = V1 V2[:, :ro] as one small GEMM up front -- the kernel without the prologue product keeps a third of
        # the LDS and three times the workgroups per CU (its main loop covers the HBM latency with resident waves alone)
        V2, ldv2, sV2 = _mat(gemm(V1, V2[:, :, :ro]))
        V1 = None
    if V1 is not None:
        V1, ldv1, sV1 = _mat(V1)
        v1p = V1.data_ptr()
    if left_out is not None:
        assert tuple(left_out.shape) == (batch, rows, ro) and left_out.is_contiguous() and left_out.dtype == M.dtype
        left = left_out
    else:
        left = torch.empty((batch, rows, ro), dtype=M.dtype, device=M.device)
    right = torch.empty((batch, ro, n), dtype=M.dtype, device=M.device)
    if batch == 0:
        return left, right
    sp, ss = None, 0
    if sigma is not None:
        sigma = sigma.contiguous()
        sp, ss = sigma.data_ptr(), sigma.shape[-1]
    _call("ttr_colproject", dt, rows, n, ro, batch, M.data_ptr(), ldm, sM, v1p, ldv1, sV1, V2.data_ptr(), ldv2, sV2, sp, ss,
          int(bool(left_ortho)), left.data_ptr(), ro, rows * ro, right.data_ptr(), n, ro * n)
    return left, right


@_on_device
def pow2_normalize(x: torch.Tensor, expo_acc: Optional[torch.Tensor] = None, exponent_only: bool = False):
    """[batch, ...] -> (x * 2^-e per batch item, e int32 [batch]) with e the binary exponent of ||x[b]||;
    ``expo_acc`` (int32 [batch]) is incremented by e in place.  ``exponent_only``: returns (None, e), x is only read."""
    dt = dtype_code(x.dtype)
    x = x.contiguous()
    batch = x.shape[0]
    count = x[0].numel() if batch > 0 else 0
    out = None if exponent_only else torch.empty_like(x)
    e = torch.empty((batch,), dtype=torch.int32, device=x.device)   # (every entry is written by the kernel)
    if batch == 0:
        return out, e
    _call("ttr_pow2_normalize", dt, count, batch, x.data_ptr(), count, _ptr(out), count, e.data_ptr(), _ptr(expo_acc))
    return out, e


@_on_device
def scale_batch(x: torch.Tensor, scale=None, expo: Optional[torch.Tensor] = None, expo_sign: int = 1) -> torch.Tensor:
    """out[b] = x[b] * scale[b] * 2^(expo_sign * expo[b]) for a [batch, ...] tensor.  ``scale``: None, a python
    number (one scalar for the whole batch) or a [batch] tensor; ``expo``: None or int32 [batch]."""
    dt = dtype_code(x.dtype)
    x = x.contiguous()
    batch = x.shape[0]
    count = x[0].numel() if batch > 0 else 0
    out = torch.empty_like(x)
    if batch == 0 or count == 0:
        return out
    sp, ss = None, 0
    if scale is not None:
        if not isinstance(scale, torch.Tensor):
            scale = torch.full((1,), float(scale), dtype=x.dtype, device=x.device)  # (a fill, not arithmetic)
            ss = 0
        else:
            scale = scale.to(x.dtype).contiguous()
            ss = 1
        sp = scale.data_ptr()
    _call("ttr_scale_batch", dt, count, batch, x.data_ptr(), count, sp, ss, _ptr(expo), int(expo_sign), out.data_ptr(), count)
    return out


@_on_device
def carry_rows32(R: torch.Tensor) -> torch.Tensor:
    """[batch, 64, cols] -> int32 [batch]: 1 where rows 32.. of R[b] are negligible by the packing test of the fused push
    (ttr_carry_rows32): the `rows32` flags of a carry that no ``qr_factor_pushed`` follows (the sweep's last core)."""
    R, ldr, sR = _mat(R)
    batch, rows, cols = R.shape
    assert rows == 64
    flag = torch.empty((batch,), dtype=torch.int32, device=R.device)
    if batch:
        _call("ttr_carry_rows32", dtype_code(R.dtype), cols, batch, R.data_ptr(), ldr, sR, flag.data_ptr())
    return flag


@_on_device
def orth_fixup(X: torch.Tensor, sigma: torch.Tensor, r: int, dead_rel: float, columns: bool = False,
               rank_dev: Optional[torch.Tensor] = None) -> None:
    """In place: orthonormal completion of the kept vectors whose sigma <= dead_rel * sigma_max (ttr_orth_fixup).
    ``X``: contiguous [batch, r, n] (rows are the vectors) or, with ``columns=True``, [batch, n, r]."""
    L = lib()
    dt = dtype_code(X.dtype)
    assert X.is_contiguous() and X.dim() == 3 and sigma.is_contiguous()
    batch = X.shape[0]
    if columns:
        n, vs, es = X.shape[1], 1, X.shape[2]
        assert X.shape[2] == r
    else:
        n, vs, es = X.shape[2], X.shape[2], 1
        assert X.shape[1] == r
    if batch == 0 or r == 0 or n == 0:
        return
    wsb = int(L.ttr_orth_fixup_workspace_bytes(dt, r, n, batch, es))   # > 0: a large batch, three launches per round
    ws = _workspace(wsb, X.device)
    _call("ttr_orth_fixup", dt, r, n, batch, X.data_ptr(), vs, es, X.shape[1] * X.shape[2], sigma.data_ptr(), sigma.shape[-1],
          float(dead_rel), _ptr(rank_dev), _ptr(ws), wsb)


@_on_device
def krp_contract(T: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """out[p, q, r] = sum_j T[p, j, q, r] * B[j, r] for contiguous T [P, J, Q, R], B [J, R]."""
    dt = dtype_code(T.dtype)
    assert T.dim() == 4 and B.dim() == 2 and T.is_cuda and T.dtype == B.dtype
    P, J, Q, R = T.shape
    assert B.shape[0] == J and B.shape[1] == R
    T = T.contiguous()
    B = B.contiguous()
    out = torch.empty((P, Q, R), dtype=T.dtype, device=T.device)
    _call("ttr_krp_contract", dt, P, J, Q, R, T.data_ptr(), B.data_ptr(), R, out.data_ptr())
    return out


@_on_device
def hadamard(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    dt = dtype_code(a.dtype)
    assert a.shape == b.shape and a.dtype == b.dtype and a.is_cuda
    a, b = a.contiguous(), b.contiguous()
    out = torch.empty_like(a)
    _call("ttr_hadamard", dt, a.numel(), a.data_ptr(), b.data_ptr(), out.data_ptr())
    return out


@_on_device
def core_kron(a: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """[B, R1, I, R2] (x) [B, S1, I, S2] -> [B, R1*S1, I, R2*S2] (slice-wise Kronecker product)."""
    dt = dtype_code(a.dtype)
    assert a.dim() == 4 and c.dim() == 4 and a.dtype == c.dtype and a.shape[0] == c.shape[0] and a.shape[2] == c.shape[2]
    a, c = a.contiguous(), c.contiguous()
    B, R1, I, R2 = a.shape
    _, S1, _, S2 = c.shape
    out = torch.empty((B, R1 * S1, I, R2 * S2), dtype=a.dtype, device=a.device)
    _call("ttr_core_kron", dt, B, R1, S1, I, R2, S2, a.data_ptr(), c.data_ptr(), out.data_ptr())
    return out


@_on_device
def gather_chain(cores, idx, out: Optional[torch.Tensor] = None, direct_max_points: int = -1) -> torch.Tensor:
    """ttr_gather_chain: cores [B, r_n, I_n, r_{n+1}] (any strides), one device index column (int32 / int64, length P, any
    stride) per core -> ``out`` [B, r_0, P, r_N] (fresh, or a given [B, r_0, P, r_N] tensor of any strides).  Raises IndexError
    when an index lies outside its mode (read from the device word the call sets; nothing else is written then)."""
    L = lib()
    n = len(cores)
    assert n >= 1 and len(idx) == n
    dt = dtype_code(cores[0].dtype)
    dev = cores[0].device
    B = cores[0].shape[0]
    P = idx[0].shape[0]
    for k in range(n):
        c = cores[k]
        assert c.dim() == 4 and c.dtype == cores[0].dtype and c.device == dev and c.shape[0] == B
        assert k == 0 or c.shape[1] == cores[k - 1].shape[3], "ttr_gather_chain: ranks do not match"
        assert idx[k].dim() == 1 and idx[k].shape[0] == P and idx[k].device == dev
    if any(i.dtype != idx[0].dtype for i in idx) or idx[0].dtype not in (torch.int32, torch.int64):
        idx = [i.to(torch.int64) for i in idx]
    ranks = (c_int64 * (n + 1))(*([int(c.shape[1]) for c in cores] + [int(cores[-1].shape[3])]))
    sizes = (c_int64 * n)(*[int(c.shape[2]) for c in cores])
    ptrs = (c_void_p * n)(*[c.data_ptr() for c in cores])
    strides = (c_int64 * (4 * n))(*[int(s) for c in cores for s in c.stride()])
    iptrs = (c_void_p * n)(*[i.data_ptr() for i in idx])
    istr = (c_int64 * n)(*[int(i.stride(0)) for i in idx])
    if out is None:
        out = torch.empty((B, ranks[0], P, ranks[n]), dtype=cores[0].dtype, device=dev)
    assert tuple(out.shape) == (B, ranks[0], P, ranks[n]) and out.dtype == cores[0].dtype
    wsb = L.ttr_gather_chain_workspace_bytes(dt, n, ranks, sizes, P, B)
    if wsb < 0:
        raise ValueError("ttr_gather_chain_workspace_bytes: bad arguments")
    ws = _workspace(wsb, dev, 1)
    flag = torch.empty(1, dtype=torch.int32, device=dev)
    _call("ttr_gather_chain", dt, n, B, P, ranks, sizes, ptrs, strides, 1 if idx[0].dtype == torch.int64 else 0, iptrs, istr,
          out.data_ptr(), *[int(s) for s in out.stride()], int(direct_max_points), flag.data_ptr(), ws.data_ptr(), wsb)
    if int(flag.item()):  # the one host read of the call
        raise IndexError("index out of range: an index array entry lies outside its mode")
    return out


@_on_device
def gather_step(X: torch.Tensor, xrow: Optional[torch.Tensor], G: torch.Tensor, idx: torch.Tensor,
                out: Optional[torch.Tensor] = None, flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ttr_gather_step: Y[p, :] = X[xrow[p], :] @ G[:, idx[p], :] for X [rows, r] (unit column stride), G [r, I, rn] (any
    strides), int64 device vectors ``xrow`` (or None: X[p]) and ``idx`` of length P -> Y [P, rn].  ``idx`` wraps negative values
    (-I <= idx < I); ``xrow`` does not (0 <= xrow < rows).  Nothing is read back: an out-of-range entry sets the device word
    ``flag`` (allocated when not given) and leaves Y unwritten."""
    dt = dtype_code(X.dtype)
    assert X.dim() == 2 and G.dim() == 3 and X.dtype == G.dtype and X.shape[1] == G.shape[0]
    if X.shape[1] > 1 and X.stride(1) != 1:
        X = X.contiguous()
    P = idx.shape[0]
    idx = idx.to(torch.int64).contiguous()
    if xrow is not None:
        xrow = xrow.to(torch.int64).contiguous()
        assert xrow.shape[0] == P
    r, I, rn = G.shape
    if out is None:
        out = torch.empty((P, rn), dtype=X.dtype, device=X.device)
    assert tuple(out.shape) == (P, rn) and (rn == 1 or out.stride(1) == 1)
    if flag is None:
        flag = torch.empty(1, dtype=torch.int32, device=X.device)
    ldx = int(X.stride(0)) if X.shape[0] > 1 else int(r)
    ldy = int(out.stride(0)) if P > 1 else int(rn)
    _call("ttr_gather_step", dt, P, X.shape[0], r, rn, I, X.data_ptr(), ldx, _ptr(xrow), G.data_ptr(),
          *[int(s) for s in G.stride()], idx.data_ptr(), out.data_ptr(), ldy, flag.data_ptr())
    return out


@_on_device
def maxvol(A: torch.Tensor, tol: float, max_iters: int, status: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """ttr_maxvol on [B, N, r] (N > r): -> index [B, r] (int64), C [B, N, r] = A A[index]^-1.  ``status`` (int32 [B, 2], optional)
    receives the done flag and the number of swaps per item."""
    L = lib()
    dt = dtype_code(A.dtype)
    A = A.contiguous()
    B, N, r = A.shape
    index = torch.empty((B, r), dtype=torch.int64, device=A.device)
    C = torch.empty((B, N, r), dtype=A.dtype, device=A.device)
    wsb = L.ttr_maxvol_workspace_bytes(dt, N, r, B)
    if wsb < 0:
        raise ValueError("ttr_maxvol_workspace_bytes: bad arguments")
    ws = torch.empty(wsb, dtype=torch.uint8, device=A.device)
    if status is not None:
        assert status.dtype == torch.int32 and status.is_contiguous() and status.numel() == 2 * B
    _call("ttr_maxvol", dt, B, N, r, A.data_ptr(), N * r, float(tol), int(max_iters), index.data_ptr(), C.data_ptr(), N * r,
          _ptr(status), ws.data_ptr(), wsb)
    return index, C


def minimize_workspace_bytes(dt: torch.dtype, M: int) -> int:
    """ttr_minimize_workspace_bytes; a negative status (a bad dtype, M < 1) is returned."""
    return int(lib().ttr_minimize_workspace_bytes(dtype_code(dt), int(M)))


@_on_device
def minimize_step(e: torch.Tensor, Ra: int, I: int, Rb: int, lset: torch.Tensor, rset: torch.Tensor, best: torch.Tensor,
                  pos: torch.Tensor, flags: torch.Tensor, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ttr_minimize_step, in place: e [Ra * I * Rb] (unit stride; a view that starts off a 16-byte boundary is taken where it
    lies) <- pi/2 - atan(e - m0), m0 = the best value so far (0 before the first), and the state ``best`` (one element of e's
    dtype), ``pos`` (int64 [nl + 1 + nr]), ``flags`` (int32 [2]: found, invalid; zeroed by the caller before the first call)
    updated from the first smallest finite entry of the original e, where that is strictly smaller than ``best`` (or nothing was
    found yet): pos = lset[a, 1:] ++ [i] ++ rset[c, :-1].  ``lset`` int64 [Ra, nl + 1], ``rset`` int64 [Rb, nr + 1], unit column
    stride, any row stride.  ``workspace``: a uint8 device tensor of at least minimize_workspace_bytes(...) bytes (allocated here
    when None).  Nothing is read back.  Returns e."""
    dt = dtype_code(e.dtype)
    Ra, I, Rb = int(Ra), int(I), int(Rb)
    M = Ra * I * Rb
    if not (e.dim() == 1 and e.shape[0] == M and (M == 1 or e.stride(0) == 1)):
        raise ValueError("minimize_step: e must be a unit-stride vector of Ra * I * Rb = {} elements".format(M))
    for name, s, rows in (("lset", lset, Ra), ("rset", rset, Rb)):
        if not (s.dim() == 2 and s.dtype == torch.int64 and s.device == e.device and s.shape[0] == rows and s.shape[1] >= 1
                and (s.shape[1] == 1 or s.stride(1) == 1) and (rows == 1 or s.stride(0) >= s.shape[1])):
            raise ValueError("minimize_step: {} must be an int64 [{}, n + 1] matrix on e's device with unit column stride".format(name, rows))
    nl, nr = lset.shape[1] - 1, rset.shape[1] - 1
    if not (best.dtype == e.dtype and best.numel() == 1 and best.device == e.device):
        raise ValueError("minimize_step: best must be one element of e's dtype on e's device")
    if not (pos.dtype == torch.int64 and pos.dim() == 1 and pos.shape[0] == nl + 1 + nr and pos.is_contiguous() and pos.device == e.device):
        raise ValueError("minimize_step: pos must be a contiguous int64 vector of nl + 1 + nr = {} elements on e's device".format(nl + 1 + nr))
    if not (flags.dtype == torch.int32 and flags.dim() == 1 and flags.shape[0] == 2 and flags.is_contiguous() and flags.device == e.device):
        raise ValueError("minimize_step: flags must be a contiguous int32 [2] vector on e's device")
    wsb = minimize_workspace_bytes(e.dtype, M)
    if wsb < 0:
        _check(wsb, "ttr_minimize_workspace_bytes")
    ws = workspace if workspace is not None else _workspace(wsb, e.device)
    _call("ttr_minimize_step", dt, e.data_ptr(), Ra, I, Rb, lset.data_ptr(), int(lset.stride(0)) if Ra > 1 else nl + 1, nl,
          rset.data_ptr(), int(rset.stride(0)) if Rb > 1 else nr + 1, nr, best.data_ptr(), pos.data_ptr(), flags.data_ptr(),
          ws.data_ptr(), int(ws.numel()))
    return e


def als_normal_groups(r0: int, r1: int) -> int:
    return int(lib().ttr_als_normal_groups(int(r0), int(r1)))


@_on_device
def als_normal(L: torch.Tensor, R: torch.Tensor, w: Optional[torch.Tensor], y: torch.Tensor, perm: torch.Tensor,
               task_begin: torch.Tensor, task_end: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """ttr_als_normal: per task t, Gp[t] = sum w_p^2 k_p k_p^T [K, K] and hp[t] = sum w_p^2 y_p k_p [K] over the samples
    perm[task_begin[t]:task_end[t]], k_p = L[p] (x) R[p] (L [P, r0], R [P, r1]); returns (Gp [T, K, K], hp [T, K])."""
    dt = dtype_code(L.dtype)
    assert L.dim() == 2 and R.dim() == 2 and L.dtype == R.dtype == y.dtype and L.shape[0] == R.shape[0]
    if L.shape[1] > 1 and L.stride(1) != 1:
        L = L.contiguous()
    if R.shape[1] > 1 and R.stride(1) != 1:
        R = R.contiguous()
    r0, r1 = int(L.shape[1]), int(R.shape[1])
    ldl = int(L.stride(0)) if L.shape[0] > 1 else r0
    ldr = int(R.stride(0)) if R.shape[0] > 1 else r1
    y = y.contiguous()
    if w is not None:
        assert w.dtype == y.dtype
        w = w.contiguous()
    T = int(task_begin.shape[0])
    assert task_begin.dtype == task_end.dtype == perm.dtype == torch.int64 and task_end.shape[0] == T
    K = r0 * r1
    Gp = torch.empty((T, K, K), dtype=L.dtype, device=L.device)
    hp = torch.empty((T, K), dtype=L.dtype, device=L.device)
    _call("ttr_als_normal", dt, T, r0, r1, L.data_ptr(), ldl, R.data_ptr(), ldr, _ptr(w), y.data_ptr(),
          perm.contiguous().data_ptr(), task_begin.contiguous().data_ptr(), task_end.contiguous().data_ptr(),
          Gp.data_ptr(), hp.data_ptr())
    return Gp, hp


def gather_grad_stage_rows(dt: torch.dtype, r0: int, r1: int) -> int:
    """Samples ttr_gather_grad stages per pass for these ranks (a multiple of 4)."""
    return int(lib().ttr_gather_grad_stage_rows(dtype_code(dt), int(r0), int(r1)))


@_on_device
def gather_grad(L: torch.Tensor, R: torch.Tensor, perm: torch.Tensor, task_begin: torch.Tensor, task_end: torch.Tensor,
                task_off: torch.Tensor, out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ttr_gather_grad: dG [r0, I, r1], dG[:, i, :] = sum over the tasks of slice i (task_off, int64 [I + 1]) of
    sum_p L[p]^T R[p] over the samples perm[task_begin[t]:task_end[t]] (L [P, r0], R [P, r1], unit column stride).  ``out``: a
    contiguous [r0, I, r1] tensor; ``workspace``: uint8, at least ttr_gather_grad_workspace_bytes (allocated when None)."""
    dt = dtype_code(L.dtype)
    assert L.dim() == 2 and R.dim() == 2 and L.dtype == R.dtype and L.shape[0] == R.shape[0]
    if L.shape[1] > 1 and L.stride(1) != 1:
        L = L.contiguous()
    if R.shape[1] > 1 and R.stride(1) != 1:
        R = R.contiguous()
    r0, r1 = int(L.shape[1]), int(R.shape[1])
    ldl = int(L.stride(0)) if L.shape[0] > 1 else r0
    ldr = int(R.stride(0)) if R.shape[0] > 1 else r1
    T = int(task_begin.shape[0])
    I = int(task_off.shape[0]) - 1
    assert task_begin.dtype == task_end.dtype == task_off.dtype == perm.dtype == torch.int64 and task_end.shape[0] == T and I >= 1
    if L.shape[0] == 0:
        T = 0  # no samples: every task is empty, and the library writes zeros for ntasks == 0
    if out is None:
        out = torch.empty((r0, I, r1), dtype=L.dtype, device=L.device)
    assert tuple(out.shape) == (r0, I, r1) and out.is_contiguous() and out.dtype == L.dtype
    wsb = int(lib().ttr_gather_grad_workspace_bytes(dt, T, r0, r1))
    if wsb < 0:
        raise ValueError("ttr_gather_grad_workspace_bytes: bad arguments")
    ws = workspace if workspace is not None else _workspace(wsb, L.device, 1)
    _call("ttr_gather_grad", dt, I, T, r0, r1, _ptr(L), ldl, _ptr(R), ldr, perm.contiguous().data_ptr(),
          task_begin.contiguous().data_ptr(), task_end.contiguous().data_ptr(), task_off.contiguous().data_ptr(), out.data_ptr(),
          ws.data_ptr(), int(ws.numel()))
    return out


def _xout(X: torch.Tensor, inner: int):
    """(item, k) -> X[item, k // inner, k % inner] for a [n_items, K // inner, inner] view X (any strides)."""
    assert X.dim() == 3 and X.shape[2] == inner
    return int(inner), int(X.stride(0)), int(X.stride(1)), int(X.stride(2))


@_on_device
def spd_solve(Gp: torch.Tensor, hp: torch.Tensor, part_off: torch.Tensor, part_base: int, X: torch.Tensor, inner: int,
              Gsum: torch.Tensor, hsum: torch.Tensor, status: torch.Tensor, counts: Optional[torch.Tensor] = None) -> None:
    """ttr_spd_solve: item i solves (sum of Gp[part_off[i] - part_base : part_off[i+1] - part_base]) x = (sum of hp ...) by Cholesky
    into X[i] (a [n_items, K // inner, inner] view, any strides); status[i] = 1 solved, 0 flagged (then Gsum[i] / hsum[i] hold the
    summed system and X[i] is not written).  ``counts`` (int64 [n], optional): samples per item; fewer than K flag the item."""
    dt = dtype_code(Gp.dtype)
    n, K = int(Gsum.shape[0]), int(Gp.shape[-1])
    assert Gp.is_contiguous() and hp.is_contiguous() and Gsum.is_contiguous() and hsum.is_contiguous()
    assert part_off.dtype == torch.int64 and part_off.is_contiguous() and part_off.shape[0] == n + 1
    assert status.dtype == torch.int32 and status.is_contiguous() and status.shape[0] == n and X.shape[0] == n
    if counts is not None:
        assert counts.dtype == torch.int64 and counts.is_contiguous() and counts.shape[0] == n
    _call("ttr_spd_solve", dt, n, K, Gp.data_ptr(), hp.data_ptr(), part_off.data_ptr(), int(part_base), X.data_ptr(),
          *_xout(X, inner), Gsum.data_ptr(), hsum.data_ptr(), status.data_ptr(), _ptr(counts))


@_on_device
def pinv_finish(V: torch.Tensor, sigma: torch.Tensor, t: torch.Tensor, status: torch.Tensor, X: torch.Tensor, inner: int) -> None:
    """ttr_pinv_finish: X[i] = V[i] diag(lambda+) t[i] for the items with status 0 (lambda = sigma^2, cut at K eps lambda_max)."""
    dt = dtype_code(V.dtype)
    n, K = int(V.shape[0]), int(V.shape[-1])
    assert V.is_contiguous() and sigma.is_contiguous() and t.is_contiguous() and t.numel() == n * K
    _call("ttr_pinv_finish", dt, n, K, V.data_ptr(), sigma.data_ptr(), t.data_ptr(), status.data_ptr(), X.data_ptr(),
          *_xout(X, inner))


RANK_NONE = 2**31 - 1   # rank cap meaning "none" (round.py:83-84)


def round_tt_plan(dt: torch.dtype, shapes, rcap, batch: int, eps_mode: bool) -> int:
    """Workspace bytes of ``round_tt_sweep`` for cores of ``shapes`` [(r0, I, r1), ...], or a negative status when the train
    lies outside the envelope of ttr_round_tt (the caller then runs its own loop over the per-kernel entries)."""
    N = len(shapes)
    sh = (c_int64 * (3 * N))(*[int(v) for s3 in shapes for v in s3])
    rc = (c_int64 * max(N - 1, 1))(*[int(r) for r in rcap])
    return int(lib().ttr_round_tt_workspace_bytes(dtype_code(dt), N, sh, rc, int(batch), int(bool(eps_mode))))


@_on_device
def round_tt_sweep(cores, rcap, algorithm: str, eps_mode: bool, eps: float, flat_thr: float, use_eigh_top: bool, outs,
                   ranks_dev: Optional[torch.Tensor], zero_flag: Optional[torch.Tensor], ws: torch.Tensor) -> None:
    """ttr_round_tt: both sweeps of tensor.py:2008-2083 on contiguous [B, r0, I, r1] ``cores`` in ONE library call; the
    rounded cores are written to ``outs`` (contiguous, at the rank caps).  See include/ttround_hip.h."""
    N = len(cores)
    B = cores[0].shape[0]
    sh = (c_int64 * (3 * N))(*[int(v) for c in cores for v in c.shape[1:]])
    rc = (c_int64 * max(N - 1, 1))(*[int(r) for r in rcap])
    cin = (c_void_p * N)(*[c.data_ptr() for c in cores])
    cout = (c_void_p * N)(*[o.data_ptr() for o in outs])
    _call("ttr_round_tt", dtype_code(cores[0].dtype), N, sh, B, cin, rc, ALG_SVD if algorithm == "svd" else ALG_EIG,
          int(bool(eps_mode)), float(eps), float(flat_thr), int(bool(use_eigh_top)), cout, _ptr(ranks_dev), _ptr(zero_flag),
          ws.data_ptr(), ws.numel())


def set_knob(knob: int, value: int):
    """Diagnostics: select a kernel variant (see ttr_debug_set_knob in the header)."""
    _check(lib().ttr_debug_set_knob(int(knob), int(value)), "ttr_debug_set_knob")


def prof_enable(on):
    """False / True: per-kind device times; 2: also the executed-work census (``prof_collect_work``)."""
    _check(lib().ttr_prof_enable(int(on)), "ttr_prof_enable")


def prof_collect_work():
    """{kind: {"flops": f, "bytes": b}} executed by the instrumented launches since the last collect (census mode)."""
    n = len(PROF_KINDS)
    fl = (c_double * n)()
    by = (c_double * n)()
    _check(lib().ttr_prof_collect_work(fl, by), "ttr_prof_collect_work")
    return {k: {"flops": fl[i], "bytes": by[i]} for i, k in enumerate(PROF_KINDS)}


def prof_collect():
    n = len(PROF_KINDS)
    ms = (c_double * n)()
    cnt = (c_int64 * n)()
    lib().ttr_prof_collect(ms, cnt)
    return {k: {"ms": ms[i], "launches": cnt[i]} for i, k in enumerate(PROF_KINDS)}


# ---------------------------------------------------------------------------------------------- sparse TT-SVD (ttr_sparse.hip)
@_on_device
def sparse_keys(X: torch.Tensor, shape_dev: torch.Tensor, flag: torch.Tensor, want_keys: bool = True) -> Optional[torch.Tensor]:
    """ttr_sparse_keys: validate X [P, N] (int64) against ``shape_dev`` (int64 [N], device) into ``flag`` (int32 [1], bit 0) and
    return the linear sort keys (x_N major, x_1 minor), or None with ``want_keys=False`` (validation only).  Nothing is read back."""
    assert X.dim() == 2 and X.dtype == torch.int64 and shape_dev.dtype == torch.int64 and flag.dtype == torch.int32
    P, N = X.shape
    key = torch.empty(P, dtype=torch.int64, device=X.device) if want_keys else None
    _call("ttr_sparse_keys", P, N, X.data_ptr(), int(X.stride(0)), int(X.stride(1)), shape_dev.data_ptr(), _ptr(key),
          flag.data_ptr())
    return key


@_on_device
def sparse_levels(X: torch.Tensor, perm: torch.Tensor, flag: torch.Tensor) -> torch.Tensor:
    """ttr_sparse_levels: int32 [P], the deepest mode (1-based) in which sample perm[p] differs from sample perm[p - 1] (N for
    p = 0, 0 and bit 1 of ``flag`` for a repeated position)."""
    assert X.dim() == 2 and X.dtype == torch.int64 and perm.dtype == torch.int32 and perm.is_contiguous()
    P, N = X.shape
    lev = torch.empty(P, dtype=torch.int32, device=X.device)
    _call("ttr_sparse_levels", P, N, X.data_ptr(), int(X.stride(0)), int(X.stride(1)), perm.data_ptr(), lev.data_ptr(),
          flag.data_ptr())
    return lev


@_on_device
def sparse_group(blk_i: torch.Tensor, I: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """ttr_sparse_group: (ilist int32 [nb], iptr int32 [I + 1]) -- the block numbers grouped by mode index ``blk_i`` (int32
    [nb]) by a stable counting sort on the device, and the group offsets."""
    L = lib()
    assert blk_i.dim() == 1 and blk_i.dtype == torch.int32 and blk_i.is_contiguous() and blk_i.is_cuda
    nb = blk_i.shape[0]
    wsb = int(L.ttr_sparse_group_workspace_bytes(nb, int(I)))
    if wsb < 0:
        _check(wsb, "ttr_sparse_group_workspace_bytes")
    ilist = torch.empty(nb, dtype=torch.int32, device=blk_i.device)
    iptr = torch.empty(I + 1, dtype=torch.int32, device=blk_i.device)
    ws = _workspace(wsb, blk_i.device, 16)
    _call("ttr_sparse_group", nb, int(I), blk_i.data_ptr(), ilist.data_ptr(), iptr.data_ptr(), ws.data_ptr(), wsb)
    return ilist, iptr


def sparse_gram_parts(dt: torch.dtype, r: int, I: int, nb: int) -> int:
    p = int(lib().ttr_sparse_gram_parts(dtype_code(dt), int(r), int(I), int(nb)))
    if p < 0:
        _check(p, "ttr_sparse_gram_parts")
    return p


@_on_device
def sparse_gram(V: torch.Tensor, I: int, colptr: torch.Tensor, blk_i: torch.Tensor, blkcol: torch.Tensor, ilist: torch.Tensor,
                iptr: torch.Tensor) -> torch.Tensor:
    """ttr_sparse_gram: G [r I, r I] = D D^T of the block table (V [nb, r]; integer device arrays colptr [C + 1], blk_i [nb],
    blkcol [nb], ilist [nb], iptr [I + 1], passed on as int32) -- see include/ttround_hip.h."""
    L = lib()
    colptr, blk_i, blkcol, ilist, iptr = (a.to(torch.int32) for a in (colptr, blk_i, blkcol, ilist, iptr))
    dt = dtype_code(V.dtype)
    assert V.dim() == 2 and (V.shape[1] == 1 or V.stride(1) == 1)
    nb, r = V.shape
    C = colptr.shape[0] - 1
    for a, n in ((colptr, C + 1), (blk_i, nb), (blkcol, nb), (ilist, nb), (iptr, I + 1)):
        assert a.is_contiguous() and a.shape[0] == n and a.device == V.device
    wsb = int(L.ttr_sparse_gram_workspace_bytes(dt, r, I, nb))
    if wsb < 0:
        _check(wsb, "ttr_sparse_gram_workspace_bytes")
    n = r * I
    G = torch.empty((n, n), dtype=V.dtype, device=V.device)
    ws = _workspace(wsb, V.device, 16)
    _call("ttr_sparse_gram", dt, r, I, nb, C, colptr.data_ptr(), blk_i.data_ptr(), blkcol.data_ptr(), ilist.data_ptr(),
          iptr.data_ptr(), V.data_ptr(), int(V.stride(0)) if nb > 1 else r, G.data_ptr(), n, ws.data_ptr(), wsb)
    return G


@_on_device
def sparse_project(V: torch.Tensor, I: int, colptr: torch.Tensor, blk_i: torch.Tensor, U: torch.Tensor, q: int) -> torch.Tensor:
    """ttr_sparse_project: W [C, q], W[c] = sum over the blocks b of column c of V[b] @ core[:, blk_i[b], :], core = U[:, :q]
    viewed as [r, I, q] (U [r I, >= q], any strides: read where it lies)."""
    dt = dtype_code(V.dtype)
    assert V.dim() == 2 and (V.shape[1] == 1 or V.stride(1) == 1) and U.dim() == 2 and U.dtype == V.dtype
    nb, r = V.shape
    C = colptr.shape[0] - 1
    assert U.shape[0] == r * I and U.shape[1] >= q
    colptr, blk_i = colptr.to(torch.int32), blk_i.to(torch.int32)
    assert colptr.is_contiguous() and blk_i.is_contiguous() and blk_i.shape[0] == nb
    W = torch.empty((C, q), dtype=V.dtype, device=V.device)
    _call("ttr_sparse_project", dt, r, I, q, nb, C, colptr.data_ptr(), blk_i.data_ptr(), V.data_ptr(),
          int(V.stride(0)) if nb > 1 else r, U.data_ptr(), int(U.stride(0)), int(U.stride(1)), W.data_ptr(), q)
    return W


def _i64(values):
    return (c_int64 * len(values))(*[int(v) for v in values])


@_on_device
def core_matvec(x: torch.Tensor, G: torch.Tensor) -> torch.Tensor:
    """ttr_core_matvec: x [P, K, Q], G [A, K, S, C] -> out [P A, S, Q C], out[p A + a, s, q C + c] = sum_k x[p, k, q] G[a, k, s, c].
    The operands are passed with the strides they have: the library refuses anything but contiguous ones."""
    dt = dtype_code(x.dtype)
    assert x.dim() == 3 and G.dim() == 4 and x.dtype == G.dtype and x.shape[1] == G.shape[1] and G.device == x.device
    P, K, Q = x.shape
    A, _, S, C = G.shape
    out = torch.empty((P * A, S, Q * C), dtype=x.dtype, device=x.device)
    _call("ttr_core_matvec", dt, P, K, Q, A, S, C, x.data_ptr(), _i64(x.stride()), G.data_ptr(), _i64(G.stride()), out.data_ptr())
    return out


def hsum_step_workspace_bytes(dt: torch.dtype, I: int, r_in, r_out) -> int:
    """ttr_hsum_step_workspace_bytes; a negative status (TTR_E_UNSUPPORTED: the ranks leave the entry's envelope) is returned."""
    return int(lib().ttr_hsum_step_workspace_bytes(dtype_code(dt), len(r_in), int(I), _i64(r_in), _i64(r_out)))


@_on_device
def hsum_step(W: torch.Tensor, cores, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ttr_hsum_step: W [r_1, .., r_K] (contiguous), cores A_m [r_m, I, r'_m] -> W' [r'_1, .., r'_K],
    W'[a'] = sum_i sum_a W[a] prod_m A_m[a_m, i, a'_m].  ``workspace``: a uint8 device tensor of at least
    hsum_step_workspace_bytes(...) bytes (allocated here when None)."""
    dt = dtype_code(W.dtype)
    K = len(cores)
    assert K >= 1 and W.dim() == K and W.is_contiguous() and all(c.dim() == 3 and c.dtype == W.dtype and c.device == W.device for c in cores)
    I = cores[0].shape[1]
    r_in, r_out = [c.shape[0] for c in cores], [c.shape[2] for c in cores]
    assert list(W.shape) == r_in and all(c.shape[1] == I for c in cores)
    wsb = hsum_step_workspace_bytes(W.dtype, I, r_in, r_out)
    if wsb < 0:
        _check(wsb, "ttr_hsum_step_workspace_bytes")
    ws = workspace if workspace is not None else _workspace(wsb, W.device)
    out = torch.empty(r_out, dtype=W.dtype, device=W.device)
    ptrs = (c_void_p * K)(*[c.data_ptr() for c in cores])
    _call("ttr_hsum_step", dt, K, I, _i64(r_in), _i64(r_out), W.data_ptr(), ptrs, _i64([s for c in cores for s in c.stride()]),
          out.data_ptr(), _ptr(ws), int(ws.numel()) if ws is not None else 0)
    return out


def mode_diff_max_order() -> int:
    """ttr_mode_diff_max_order: the number of passes ttr_mode_diff fuses into one launch."""
    return int(lib().ttr_mode_diff_max_order())


@_on_device
def mode_diff(X: torch.Tensor, order: int, periodic: bool, inv_step: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ttr_mode_diff: Y = (inv_step S)^order X along the middle axis of X [R, I, C].  ``out``: a [R, I, C] view with element
    strides (sr, si, 1) that receives the result (e.g. a block of a wider core); a fresh contiguous tensor when None.  X is passed
    with the strides it has: the library refuses anything but contiguous ones.  Orders above the fused limit are chained here:
    full launches into contiguous temporaries, the last one into ``out``."""
    dt = dtype_code(X.dtype)
    assert X.dim() == 3 and (out is None or (tuple(out.shape) == tuple(X.shape) and out.dtype == X.dtype and out.device == X.device))
    R, I, C = X.shape
    order = int(order)
    Y = out if out is not None else torch.empty((R, I, C), dtype=X.dtype, device=X.device)
    left = max(order, 1)
    fused = mode_diff_max_order()
    while True:
        o = order if order < 1 else min(left, fused)   # (a bad order goes to the library as it is: TTR_E_INVALID)
        left -= o
        dst = Y if left <= 0 else torch.empty((R, I, C), dtype=X.dtype, device=X.device)
        _call("ttr_mode_diff", dt, R, I, C, o, int(bool(periodic)), float(inv_step), X.data_ptr(), _i64(X.stride()), dst.data_ptr(),
              _i64(dst.stride()))
        if left <= 0:
            return Y
        X = dst


@_on_device
def laplace_core(X: torch.Tensor, pos: int, periodic: bool, inv_step: float) -> torch.Tensor:
    """ttr_laplace_core: X [R, I, C] -> [X D] (pos 0, [R, I, 2C]), [[X, D], [0, X]] (pos 1, [2R, I, 2C]) or [D ; X] (pos 2,
    [2R, I, C]) with D = (inv_step S)^2 X, one launch."""
    dt = dtype_code(X.dtype)
    assert X.dim() == 3
    R, I, C = X.shape
    shape = {0: (R, I, 2 * C), 1: (2 * R, I, 2 * C), 2: (2 * R, I, C)}.get(int(pos), (2 * R, I, 2 * C))
    out = torch.empty(shape, dtype=X.dtype, device=X.device)
    _call("ttr_laplace_core", dt, R, I, C, int(pos), int(bool(periodic)), float(inv_step), X.data_ptr(), _i64(X.stride()), out.data_ptr())
    return out


@_on_device
def mode_scan(X: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ttr_mode_scan: Y[r, i, c] = sum_{i' <= i} X[r, i', c] for X [R, I, C].  ``out``: a [R, I, C] view with element strides
    (sr, si, 1) that receives the result (e.g. a block of a wider core); a fresh contiguous tensor when None.  X is passed with
    the strides it has: the library refuses anything but contiguous ones."""
    dt = dtype_code(X.dtype)
    assert X.dim() == 3 and (out is None or (tuple(out.shape) == tuple(X.shape) and out.dtype == X.dtype and out.device == X.device))
    R, I, C = X.shape
    Y = out if out is not None else torch.empty((R, I, C), dtype=X.dtype, device=X.device)
    _call("ttr_mode_scan", dt, R, I, C, X.data_ptr(), _i64(X.stride()), Y.data_ptr(), _i64(Y.stride()))
    return Y


@_on_device
def mode_reduce(X: torch.Tensor, w: Optional[torch.Tensor] = None, scale: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ttr_mode_reduce: Y[r, c] = scale * sum_i w[i] X[r, i, c] for X [R, I, C]; ``w``: [I] contiguous elements of X's dtype on its
    device, or None (all ones).  ``out``: a [R, C] view with element strides (sr, 1) that receives the result; a fresh contiguous
    tensor when None.  X is passed with the strides it has: the library refuses anything but contiguous ones."""
    dt = dtype_code(X.dtype)
    assert X.dim() == 3 and (out is None or (tuple(out.shape) == (X.shape[0], X.shape[2]) and out.dtype == X.dtype and out.device == X.device))
    R, I, C = X.shape
    if w is not None and not (w.dim() == 1 and w.shape[0] == I and w.dtype == X.dtype and w.device == X.device and w.is_contiguous()):
        raise ValueError("mode_reduce: w must be a contiguous vector of {} elements of X's dtype on X's device".format(I))
    Y = out if out is not None else torch.empty((R, C), dtype=X.dtype, device=X.device)
    _call("ttr_mode_reduce", dt, R, I, C, X.data_ptr(), _i64(X.stride()), _ptr(w), float(scale), Y.data_ptr(), _i64(Y.stride()))
    return Y


def mode_sandwich_max_rank() -> int:
    """ttr_mode_sandwich_max_rank: the largest R and C ttr_mode_sandwich takes."""
    return int(lib().ttr_mode_sandwich_max_rank())


def mode_sandwich_workspace_bytes(dt: torch.dtype, S: int, R: int, I: int, C: int) -> int:
    """ttr_mode_sandwich_workspace_bytes; a negative status (the entry would refuse these sizes) is returned."""
    return int(lib().ttr_mode_sandwich_workspace_bytes(dtype_code(dt), int(S), int(R), int(I), int(C)))


@_on_device
def mode_sandwich(Z: torch.Tensor, A: torch.Tensor, w: Optional[torch.Tensor] = None, mu: Optional[torch.Tensor] = None,
                  workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ttr_mode_sandwich: Z [S, R, R] (contiguous), A [R, I, C], w [I] or None (ones), mu [R, C] or None (zeros) -> Q [S, C, C],
    Q[s] = sum_i w[i] (A_i - mu)^T Z[s] (A_i - mu).  A is passed with the strides it has: the library refuses anything but
    contiguous ones.  ``workspace``: a uint8 device tensor of at least mode_sandwich_workspace_bytes(...) bytes (allocated here
    when None)."""
    dt = dtype_code(Z.dtype)
    assert Z.dim() == 3 and A.dim() == 3 and Z.is_contiguous() and A.dtype == Z.dtype and A.device == Z.device
    S, R, _ = Z.shape
    _, I, C = A.shape
    assert Z.shape[2] == R and A.shape[0] == R
    if w is not None and not (w.dim() == 1 and w.shape[0] == I and w.dtype == Z.dtype and w.device == Z.device and w.is_contiguous()):
        raise ValueError("mode_sandwich: w must be a contiguous vector of {} elements of Z's dtype on Z's device".format(I))
    if mu is not None and not (tuple(mu.shape) == (R, C) and mu.dtype == Z.dtype and mu.device == Z.device and mu.is_contiguous()):
        raise ValueError("mode_sandwich: mu must be a contiguous [{}, {}] matrix of Z's dtype on Z's device".format(R, C))
    wsb = mode_sandwich_workspace_bytes(Z.dtype, S, R, I, C)
    if wsb < 0:
        _check(wsb, "ttr_mode_sandwich_workspace_bytes")
    ws = workspace if workspace is not None else _workspace(wsb, Z.device)
    Q = torch.empty((S, C, C), dtype=Z.dtype, device=Z.device)
    _call("ttr_mode_sandwich", dt, S, R, I, C, Z.data_ptr(), A.data_ptr(), _i64(A.stride()), _ptr(w), _ptr(mu), Q.data_ptr(), _ptr(ws),
          int(ws.numel()) if ws is not None else 0)
    return Q


def pce_max_order() -> int:
    """ttr_pce_max_order: the largest number S of basis polynomials per mode ttr_pce_design / ttr_pce_predict take."""
    return int(lib().ttr_pce_max_order())


def pce_max_basis() -> int:
    """ttr_pce_max_basis: the largest N * S ttr_pce_design / ttr_pce_predict take."""
    return int(lib().ttr_pce_max_basis())


def _pce_args(who: str, Z: torch.Tensor, Psi: torch.Tensor, coords: torch.Tensor, flag: Optional[torch.Tensor]):
    if not (isinstance(Z, torch.Tensor) and Z.is_cuda and Z.dim() == 2):
        raise ValueError("{}: Z must be a [P, N] device matrix".format(who))
    P, N = Z.shape
    if not (Psi.dim() == 3 and Psi.shape[0] == N and Psi.shape[1] == Psi.shape[2] and Psi.dtype == Z.dtype and Psi.device == Z.device
            and Psi.is_contiguous()):
        raise ValueError("{}: Psi must be a contiguous [N, S, S] tensor of Z's dtype on Z's device".format(who))
    if not (coords.dim() == 2 and coords.shape[1] == N and coords.dtype == torch.int64 and coords.device == Z.device and coords.is_contiguous()):
        raise ValueError("{}: coords must be a contiguous int64 [C, N] tensor on Z's device".format(who))
    if flag is None:
        flag = torch.zeros(1, dtype=torch.int32, device=Z.device)
    elif not (flag.dtype == torch.int32 and flag.numel() == 1 and flag.device == Z.device):
        raise ValueError("{}: flag must be one int32 on Z's device".format(who))
    return P, N, int(Psi.shape[1]), int(coords.shape[0]), flag


@_on_device
def pce_design(Z: torch.Tensor, Psi: torch.Tensor, coords: torch.Tensor, out: Optional[torch.Tensor] = None,
               flag: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """ttr_pce_design: M[p, c] = prod_n B(p, n, coords[c, n]) with B(p, n, s) = sum_k Z[p, n]^k Psi[n, k, s], for Z [P, N] (any
    element strides), Psi [N, S, S] and coords [C, N] (int64).  ``out``: a [P, C] view with element strides (ldm, 1) that receives
    the result; a fresh contiguous matrix when None.  Returns (M, flag): ``flag`` (one int32 on the device, zeroed here when not
    given) has bit 0 set where a coordinate lay outside [0, S) -- that candidate's column is 0.  Nothing is read back."""
    dt = dtype_code(Z.dtype)
    P, N, S, C, flag = _pce_args("pce_design", Z, Psi, coords, flag)
    if out is not None and not (tuple(out.shape) == (P, C) and out.dtype == Z.dtype and out.device == Z.device
                                and (C <= 1 or out.stride(1) == 1) and (P <= 1 or out.stride(0) >= C)):
        raise ValueError("pce_design: out must be a [P, C] view of Z's dtype with element strides (ldm >= C, 1)")
    M = out if out is not None else torch.empty((P, C), dtype=Z.dtype, device=Z.device)
    if P == 0 or C == 0:
        return M, flag
    ldm = int(M.stride(0)) if P > 1 else C
    _call("ttr_pce_design", dt, P, N, S, C, Z.data_ptr(), int(Z.stride(0)), int(Z.stride(1)), Psi.data_ptr(), coords.data_ptr(),
          M.data_ptr(), ldm, flag.data_ptr())
    return M, flag


@_on_device
def pce_predict(Z: torch.Tensor, Psi: torch.Tensor, coords: torch.Tensor, coef: torch.Tensor,
                flag: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """ttr_pce_predict: y[p] = sum_c coef[c] prod_n B(p, n, coords[c, n]) (arguments as for ``pce_design``, ``coef`` [C]
    contiguous, of Z's dtype); the P x C matrix is never formed.  Returns (y, flag).  Nothing is read back."""
    dt = dtype_code(Z.dtype)
    P, N, S, C, flag = _pce_args("pce_predict", Z, Psi, coords, flag)
    if not (coef.dim() == 1 and coef.shape[0] == C and coef.dtype == Z.dtype and coef.device == Z.device and coef.is_contiguous()):
        raise ValueError("pce_predict: coef must be a contiguous vector of {} elements of Z's dtype on Z's device".format(C))
    if P == 0 or C == 0:
        return torch.zeros(P, dtype=Z.dtype, device=Z.device), flag
    y = torch.empty(P, dtype=Z.dtype, device=Z.device)
    _call("ttr_pce_predict", dt, P, N, S, C, Z.data_ptr(), int(Z.stride(0)), int(Z.stride(1)), Psi.data_ptr(), coords.data_ptr(),
          coef.data_ptr(), y.data_ptr(), flag.data_ptr())
    return y, flag



def core_convolve_max_taps() -> int:
    """ttr_core_convolve_max_taps: the terms of the sum ttr_core_convolve stages in LDS at once (longer sums are chunked)."""
    return int(lib().ttr_core_convolve_max_taps())


@_on_device
def core_convolve(a: torch.Tensor, c: torch.Tensor, lo: int, K: int) -> torch.Tensor:
    """ttr_core_convolve: a [R1, I, R2], c [S1, J, S2] (contiguous) -> [R1 S1, K, R2 S2] with
    out[r1 S1 + s1, k, r2 S2 + s2] = sum_i a[r1, i, r2] c[s1, k + lo - i, s2]: the window (lo, K) of the full result of
    I + J - 1 entries.  ValueError for anything but two contiguous 3-d device cores of one dtype, or a window the library refuses."""
    if a.dim() != 3 or c.dim() != 3 or a.dtype != c.dtype or a.device != c.device or not a.is_cuda:
        raise ValueError("core_convolve: expected two 3-d cores of one dtype on one device")
    if not (a.is_contiguous() and c.is_contiguous()):
        raise ValueError("core_convolve: the cores must be contiguous")
    dt = dtype_code(a.dtype)
    R1, I, R2 = a.shape
    S1, J, S2 = c.shape
    lo, K = int(lo), int(K)
    out = torch.empty((R1 * S1, max(K, 0), R2 * S2), dtype=a.dtype, device=a.device)
    _call("ttr_core_convolve", dt, R1, I, R2, S1, J, S2, lo, K, a.data_ptr(), c.data_ptr(), out.data_ptr())
    return out


@_on_device
def core_compose(A: torch.Tensor, B: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ttr_core_compose: A [R1, P, J, R2], B [S1, J, Q, S2] (contiguous) -> [R1 S1, P, Q, R2 S2] with
    out[r S1 + a, p, q, s S2 + b] = sum_j A[r, p, j, s] B[a, j, q, b]: one core of a TT-matrix product that stays in TT format.
    ValueError for anything but two contiguous 4-d device cores of one dtype with the same J.  ``out``: a contiguous tensor of
    that many elements which receives the result (wherever it lies: the bits do not depend on its alignment); fresh when None."""
    if A.dim() != 4 or B.dim() != 4 or A.dtype != B.dtype or A.device != B.device or not A.is_cuda:
        raise ValueError("core_compose: expected two 4-d cores of one dtype on one device")
    if A.shape[2] != B.shape[1]:
        raise ValueError("core_compose: A [R1, P, J, R2] and B [S1, J, Q, S2] need the same J, got {} and {}".format(A.shape[2], B.shape[1]))
    if not (A.is_contiguous() and B.is_contiguous()):
        raise ValueError("core_compose: the cores must be contiguous")
    dt = dtype_code(A.dtype)
    R1, P, J, R2 = A.shape
    S1, _, Q, S2 = B.shape
    shape = (R1 * S1, P, Q, R2 * S2)
    if out is None:
        out = torch.empty(shape, dtype=A.dtype, device=A.device)
    if not (out.numel() == R1 * S1 * P * Q * R2 * S2 and out.is_contiguous() and out.dtype == A.dtype and out.device == A.device):
        raise ValueError("core_compose: out must be a contiguous tensor of {} elements of the cores' dtype on their device".format(
            R1 * S1 * P * Q * R2 * S2))
    _call("ttr_core_compose", dt, R1, P, J, R2, S1, Q, S2, A.data_ptr(), B.data_ptr(), out.data_ptr())
    return out.view(shape)


def accept_max_rank() -> int:
    """ttr_accept_max_rank: the largest rank ttr_accept_count / ttr_accept_expand take."""
    return int(lib().ttr_accept_max_rank())


def _accept_arg(x: torch.Tensor, dtype, shape, name: str):
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == dtype and tuple(x.shape) == tuple(shape) and x.is_contiguous()):
        raise ValueError("accept: {} must be a contiguous {} device tensor of shape {}".format(name, dtype, tuple(shape)))


@_on_device
def accept_count(L: torch.Tensor, fiber: torch.Tensor) -> torch.Tensor:
    """ttr_accept_count: L [P, r] (fp64), fiber [r, I] (fp32 or fp64) -> C [P, I] int64, C = rint(L @ fiber) accumulated in fp64.
    ValueError for a rank above accept_max_rank()."""
    dt = dtype_code(fiber.dtype)
    if L.dim() != 2 or fiber.dim() != 2:
        raise ValueError("accept_count: expected L [P, r] and fiber [r, I]")
    P, r = L.shape
    I = fiber.shape[1]
    _accept_arg(L, torch.float64, (P, r), "L")
    _accept_arg(fiber, fiber.dtype, (r, I), "fiber")
    C = torch.empty((P, I), dtype=torch.int64, device=L.device)
    _call("ttr_accept_count", dt, P, r, I, L.data_ptr(), fiber.data_ptr(), C.data_ptr())
    return C


@_on_device
def accept_expand(L: torch.Tensor, core: torch.Tensor, C: torch.Tensor, childoff: torch.Tensor, cnt: torch.Tensor, idx: torch.Tensor,
                  Xs: torch.Tensor, mu: int, flag: torch.Tensor, last: bool):
    """ttr_accept_expand: the K = len(idx) listed children of the frontier (L [P, r] fp64, C / childoff [P, I], cnt [P]) through
    core [r, I, r'] -> (Lnew [K, r'] fp64 or None when ``last``, offnew [K], cntnew [K]); column ``mu`` of Xs [S, N] is filled and
    ``flag`` (int32 [1]) ORed.  ValueError for a rank above accept_max_rank()."""
    dt = dtype_code(core.dtype)
    if L.dim() != 2 or core.dim() != 3 or Xs.dim() != 2 or idx.dim() != 1:
        raise ValueError("accept_expand: expected L [P, r], core [r, I, r'], idx [K] and Xs [S, N]")
    P, r = L.shape
    I, rn = core.shape[1], core.shape[2]
    K, (S, N) = idx.shape[0], Xs.shape
    _accept_arg(L, torch.float64, (P, r), "L")
    _accept_arg(core, core.dtype, (r, I, rn), "core")
    _accept_arg(C, torch.int64, (P, I), "C")
    _accept_arg(childoff, torch.int64, (P, I), "childoff")
    _accept_arg(cnt, torch.int64, (P,), "cnt")
    _accept_arg(idx, torch.int64, (K,), "idx")
    _accept_arg(Xs, torch.int64, (S, N), "Xs")
    _accept_arg(flag, torch.int32, (1,), "flag")
    Lnew = None if last else torch.empty((K, rn), dtype=torch.float64, device=L.device)
    offnew = torch.empty((K,), dtype=torch.int64, device=L.device)
    cntnew = torch.empty((K,), dtype=torch.int64, device=L.device)
    _call("ttr_accept_expand", dt, P, r, I, rn, K, N, int(mu), S, L.data_ptr(), core.data_ptr(), C.data_ptr(), childoff.data_ptr(),
          cnt.data_ptr(), idx.data_ptr(), _ptr(Lnew), offnew.data_ptr(), cntnew.data_ptr(), Xs.data_ptr(), flag.data_ptr())
    return Lnew, offnew, cntnew


def sample_max_rank() -> int:
    """ttr_sample_max_rank: the largest rank ttr_sample_step takes."""
    return int(lib().ttr_sample_max_rank())


def sample_tile(dt: torch.dtype) -> Tuple[int, int]:
    """(S, B) of ttr_sample_step in this dtype: the samples a workgroup owns and the columns of fiber per block
    (TTR_SAMPLE_TILE_* / TTR_SAMPLE_BLOCK_* of the header)."""
    return (SAMPLE_TILE_F32, SAMPLE_BLOCK_F32) if dtype_code(dt) == F32 else (SAMPLE_TILE_F64, SAMPLE_BLOCK_F64)


@_on_device
def sample_step(L: torch.Tensor, fiber: torch.Tensor, core: torch.Tensor, u: torch.Tensor, x: torch.Tensor, flag: torch.Tensor,
                Lnew: Optional[torch.Tensor] = None) -> None:
    """ttr_sample_step: one mode of the sampling sweep for the P rows of L [P, r] (unit column stride, any row stride >= r):
    x[p] (int64 [P], any stride: a column of Xs) = the index drawn with the threshold u[p] (fp64 [P], any stride) from
    q = |L[p, :] @ fiber| (fiber [r, I] contiguous), and Lnew[p, :] = (L[p, :] @ core[:, x[p], :]) / sum q when ``Lnew``
    ([P, r'], unit column stride) is given.  ``core`` [r, I, r'] is taken with its own strides (the entry refuses what it does
    not take: NotImplementedError).  ``flag`` (int32 [1]) is ORed with SAMPLE_* bits; nothing is read back.  ValueError for a
    rank above sample_max_rank()."""
    dt = dtype_code(core.dtype)
    if L.dim() != 2 or fiber.dim() != 2 or core.dim() != 3 or u.dim() != 1 or x.dim() != 1:
        raise ValueError("sample_step: expected L [P, r], fiber [r, I], core [r, I, r'], u [P] and x [P]")
    P, r = L.shape
    I, rn = core.shape[1], core.shape[2]
    tensors = [L, fiber, core, u, x, flag] + ([Lnew] if Lnew is not None else [])
    if not all(t.is_cuda and t.device == core.device for t in tensors):
        raise ValueError("sample_step: every operand must be on the core's device")
    if not (L.dtype == core.dtype and fiber.dtype == core.dtype and tuple(fiber.shape) == (r, I) and fiber.is_contiguous()
            and core.shape[0] == r and (r == 1 or L.stride(1) == 1)):
        raise ValueError("sample_step: L [P, r] (unit column stride) and a contiguous fiber [r, I] of the core's dtype are needed")
    if not (u.dtype == torch.float64 and u.shape[0] == P and x.dtype == torch.int64 and x.shape[0] == P):
        raise ValueError("sample_step: u must be fp64 [P] and x int64 [P]")
    if not (flag.dtype == torch.int32 and flag.numel() == 1):
        raise ValueError("sample_step: flag must be one int32 word")
    if Lnew is not None and not (Lnew.dtype == core.dtype and tuple(Lnew.shape) == (P, rn) and (rn == 1 or Lnew.stride(1) == 1)):
        raise ValueError("sample_step: Lnew must be [P, r'] of the core's dtype with unit column stride")
    cs = (c_int64 * 3)(*[int(s) for s in core.stride()])
    _call("ttr_sample_step", dt, P, r, I, rn, L.data_ptr(), int(L.stride(0)) if P > 1 else r, fiber.data_ptr(), core.data_ptr(), cs,
          u.data_ptr(), int(u.stride(0)) if P > 1 else 1, x.data_ptr(), int(x.stride(0)) if P > 1 else 1, _ptr(Lnew),
          (int(Lnew.stride(0)) if P > 1 else rn) if Lnew is not None else rn, flag.data_ptr())


@_on_device
def ttm_step(X: torch.Tensor, G: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ttr_ttm_step: X [I, D, R], G [R, I, O, S] (a TTMatrix core) -> Y [D, O, S], Y[dd, o, s] = sum_i sum_r X[i, dd, r] G[r, i, o, s].
    The operands are passed with the strides they have: the library refuses anything but contiguous ones (NotImplementedError).
    ``out``: a contiguous tensor of D O S elements that receives the result (its shape is not looked at: the caller reads it as
    the next step's X); a fresh [D, O, S] tensor when None."""
    dt = dtype_code(X.dtype)
    assert X.dim() == 3 and G.dim() == 4 and G.dtype == X.dtype and G.device == X.device
    I, D, R = X.shape
    assert G.shape[0] == R and G.shape[1] == I
    O, S = G.shape[2], G.shape[3]
    if out is None:
        out = torch.empty((D, O, S), dtype=X.dtype, device=X.device)
    assert out.numel() == D * O * S and out.is_contiguous() and out.dtype == X.dtype and out.device == X.device
    _call("ttr_ttm_step", dt, I, D, R, O, S, X.data_ptr(), _i64(X.stride()), G.data_ptr(), _i64(G.stride()), out.data_ptr())
    return out


@_on_device
def cpm_step(X: torch.Tensor, C: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ttr_cpm_step: X [I, D, R] (or [I, D]: the first step, broadcast over r), C [I, O, R] (a CPMatrix core) -> Y [D, O, R],
    Y[dd, o, r] = sum_i X[i, dd, r] C[i, o, r].  The entry takes contiguous operands only (it has no stride arguments), so
    anything else is refused here (ValueError).  ``out``: a contiguous tensor of D O R elements; a fresh [D, O, R] tensor when None."""
    dt = dtype_code(X.dtype)
    assert X.dim() in (2, 3) and C.dim() == 3 and C.dtype == X.dtype and C.device == X.device
    I, O, R = C.shape
    D = X.shape[1]
    assert X.shape[0] == I and (X.dim() == 2 or X.shape[2] == R)
    if not (X.is_contiguous() and C.is_contiguous()):
        raise ValueError("cpm_step: X and C must be contiguous")
    if out is None:
        out = torch.empty((D, O, R), dtype=X.dtype, device=X.device)
    assert out.numel() == D * O * R and out.is_contiguous() and out.dtype == X.dtype and out.device == X.device
    _call("ttr_cpm_step", dt, I, D, O, R, int(X.dim() == 3), X.data_ptr(), C.data_ptr(), out.data_ptr())
    return out


@_on_device
def ttm_grad_input(dY: torch.Tensor, G: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ttr_ttm_grad_input: dY (D O S elements, read as [D, O, S]), G [R, I, O, S] (a TTMatrix core) -> dX [I, D, R],
    dX[i, dd, r] = sum_{o, s} dY[dd, o, s] G[r, i, o, s]: the gradient of ttm_step's X.  The entry takes contiguous operands only
    (it has no stride arguments), so anything else is refused here (ValueError).  ``out``: a contiguous tensor of I D R elements
    (its shape is not looked at: the caller reads it as the previous step's dY); a fresh [I, D, R] tensor when None."""
    dt = dtype_code(G.dtype)
    assert G.dim() == 4 and dY.dtype == G.dtype and dY.device == G.device
    R, I, O, S = G.shape
    assert dY.numel() % (O * S) == 0
    D = dY.numel() // (O * S)
    if not (dY.is_contiguous() and G.is_contiguous()):
        raise ValueError("ttm_grad_input: dY and G must be contiguous")
    if out is None:
        out = torch.empty((I, D, R), dtype=G.dtype, device=G.device)
    assert out.numel() == I * D * R and out.is_contiguous() and out.dtype == G.dtype and out.device == G.device
    _call("ttr_ttm_grad_input", dt, I, D, R, O, S, dY.data_ptr(), G.data_ptr(), out.data_ptr())
    return out


def ttm_grad_core_slab_rows(dt: torch.dtype, I: int, D: int, R: int, O: int, S: int) -> int:
    """Rows of D one workgroup of ttr_ttm_grad_core sums (a function of these six arguments only)."""
    return int(lib().ttr_ttm_grad_core_slab_rows(dtype_code(dt), int(I), int(D), int(R), int(O), int(S)))


def ttm_grad_core_workspace_bytes(dt: torch.dtype, I: int, D: int, R: int, O: int, S: int) -> int:
    """Bytes of workspace ttr_ttm_grad_core needs for these sizes (0 where D is one slab)."""
    return int(lib().ttr_ttm_grad_core_workspace_bytes(dtype_code(dt), int(I), int(D), int(R), int(O), int(S)))


@_on_device
def ttm_grad_core(X: torch.Tensor, dY: torch.Tensor, out: Optional[torch.Tensor] = None,
                  workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ttr_ttm_grad_core: X [I, D, R], dY (D N elements, read as [D, N]; N = O S is taken from ``out``, or is dY.shape[1:] when
    ``out`` is None and dY is [D, O, S]) -> dG [R, I, O, S], dG[r, i, o, s] = sum_dd X[i, dd, r] dY[dd, o, s]: the gradient of
    ttm_step's G.  Contiguous operands only (ValueError otherwise).  ``out``: a contiguous [R, I, O, S] tensor; ``workspace``:
    uint8, at least ttr_ttm_grad_core_workspace_bytes (allocated when None and needed)."""
    dt = dtype_code(X.dtype)
    assert X.dim() == 3 and dY.dtype == X.dtype and dY.device == X.device
    I, D, R = X.shape
    if out is None:
        assert dY.dim() == 3 and dY.shape[0] == D
        out = torch.empty((R, I, dY.shape[1], dY.shape[2]), dtype=X.dtype, device=X.device)
    assert out.dim() == 4 and out.shape[0] == R and out.shape[1] == I and out.is_contiguous() and out.dtype == X.dtype and out.device == X.device
    O, S = out.shape[2], out.shape[3]
    assert dY.numel() == D * O * S
    if not (X.is_contiguous() and dY.is_contiguous()):
        raise ValueError("ttm_grad_core: X and dY must be contiguous")
    wsb = int(lib().ttr_ttm_grad_core_workspace_bytes(dt, I, D, R, O, S))
    if wsb < 0:
        _check(wsb, "ttr_ttm_grad_core_workspace_bytes")
    ws = workspace if workspace is not None else _workspace(wsb, X.device)
    _call("ttr_ttm_grad_core", dt, I, D, R, O, S, X.data_ptr(), dY.data_ptr(), out.data_ptr(), _ptr(ws),
          int(ws.numel()) if ws is not None else 0)
    return out


def ttm_lookup_workspace_bytes(P: int, I: int) -> int:
    """Bytes of workspace ttr_ttm_lookup_step needs for P samples and a mode of size I (the grouping of the samples)."""
    wsb = int(lib().ttr_ttm_lookup_workspace_bytes(int(P), int(I)))
    if wsb < 0:
        _check(wsb, "ttr_ttm_lookup_workspace_bytes")
    return wsb


@_on_device
def ttm_lookup_step(X: torch.Tensor, xrow: Optional[torch.Tensor], G: torch.Tensor, idx: torch.Tensor, flag: torch.Tensor,
                    out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ttr_ttm_lookup_step: Y[p, dd, o, s] = sum_r X[xrow[p], dd, r] G[r, idx[p], o, s] for a contiguous X [rows_x, D, R], G
    [R, I, O, S] (a TTMatrix core, passed with the strides it has: the library wants a unit last stride) and int64 device vectors
    ``idx`` and ``xrow`` (or None: X[p]) of P entries WITH THE SAME STRIDE (two columns of one digit table, or two contiguous
    vectors) -> Y [P, D, O, S].  ``idx`` wraps negative values, ``xrow`` does not.  Nothing is read back: a bad entry ORs the
    int32 device word ``flag`` and leaves Y unwritten, and so does a word that is set on entry; the word is never cleared here.
    ``out``: a contiguous tensor of P D O S elements; ``workspace``: uint8, at least ``ttm_lookup_workspace_bytes(P, I)``."""
    dt = dtype_code(X.dtype)
    assert X.dim() == 3 and G.dim() == 4 and G.dtype == X.dtype and G.device == X.device and X.is_contiguous()
    rows_x, D, R = X.shape
    assert G.shape[0] == R
    I, O, S = G.shape[1], G.shape[2], G.shape[3]
    assert idx.dim() == 1 and idx.dtype == torch.int64 and idx.device == X.device
    P = idx.shape[0]
    stride = int(idx.stride(0)) if P > 1 else 1
    if xrow is not None:
        assert xrow.dtype == torch.int64 and tuple(xrow.shape) == (P,) and xrow.device == X.device
        assert P <= 1 or int(xrow.stride(0)) == stride, "ttm_lookup_step: idx and xrow must have the same stride"
    assert flag.dtype == torch.int32 and flag.numel() == 1 and flag.device == X.device
    if out is None:
        out = torch.empty((P, D, O, S), dtype=X.dtype, device=X.device)
    assert out.numel() == P * D * O * S and out.is_contiguous() and out.dtype == X.dtype and out.device == X.device
    if P == 0:
        return out
    ws = workspace if workspace is not None else _workspace(ttm_lookup_workspace_bytes(P, I), X.device)
    _call("ttr_ttm_lookup_step", dt, P, rows_x, D, R, I, O, S, X.data_ptr(), _ptr(xrow), G.data_ptr(), _i64(G.stride()),
          idx.data_ptr(), stride, out.data_ptr(), flag.data_ptr(), ws.data_ptr(), int(ws.numel()))
    return out


def ttm_lookup_grad_core_slab_rows(dt: torch.dtype, P: int, D: int, R: int, I: int, O: int, S: int) -> int:
    """K rows (sample, dd) one workgroup of ttr_ttm_lookup_grad_core sums (a function of these seven arguments only)."""
    rows = int(lib().ttr_ttm_lookup_grad_core_slab_rows(dtype_code(dt), int(P), int(D), int(R), int(I), int(O), int(S)))
    if rows < 0:
        _check(rows, "ttr_ttm_lookup_grad_core_slab_rows")
    return rows


def ttm_lookup_grad_core_workspace_bytes(dt: torch.dtype, P: int, D: int, R: int, I: int, O: int, S: int) -> int:
    """Bytes of workspace ttr_ttm_lookup_grad_core needs: the counts and ceil(P D / slab_rows) + I partial tiles."""
    wsb = int(lib().ttr_ttm_lookup_grad_core_workspace_bytes(dtype_code(dt), int(P), int(D), int(R), int(I), int(O), int(S)))
    if wsb < 0:
        _check(wsb, "ttr_ttm_lookup_grad_core_workspace_bytes")
    return wsb


def ttm_lookup_grad_input_workspace_bytes(P: int, I: int) -> int:
    """Bytes of workspace ttr_ttm_lookup_grad_input needs for a mode of size I (the counts of the groups)."""
    wsb = int(lib().ttr_ttm_lookup_grad_input_workspace_bytes(int(P), int(I)))
    if wsb < 0:
        _check(wsb, "ttr_ttm_lookup_grad_input_workspace_bytes")
    return wsb


def _lookup_grad_indices(who: str, idx: torch.Tensor, perm: torch.Tensor, xrow: Optional[torch.Tensor], flag: torch.Tensor, device):
    """(P, stride) of the index operands of the two gradient entries, checked as ttm_lookup_step checks them."""
    assert idx.dim() == 1 and idx.dtype == torch.int64 and idx.device == device, who
    P = idx.shape[0]
    stride = int(idx.stride(0)) if P > 1 else 1
    assert perm.dtype == torch.int64 and tuple(perm.shape) == (P,) and perm.device == device and perm.is_contiguous(), who
    if xrow is not None:
        assert xrow.dtype == torch.int64 and tuple(xrow.shape) == (P,) and xrow.device == device
        assert P <= 1 or int(xrow.stride(0)) == stride, who + ": idx and xrow must have the same stride"
    assert flag.dtype == torch.int32 and flag.numel() == 1 and flag.device == device
    return P, stride


@_on_device
def ttm_lookup_grad_core(X: torch.Tensor, xrow: Optional[torch.Tensor], dY: torch.Tensor, idx: torch.Tensor, perm: torch.Tensor,
                         flag: torch.Tensor, out: torch.Tensor, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ttr_ttm_lookup_grad_core: dG[r, i, o, s] = sum_{p: idx[p] = i} sum_dd X[xrow[p], dd, r] dY[p, dd, o, s] for a contiguous X
    [rows_x, D, R] and dY (P D O S contiguous elements, read as [P, D, O, S]) into ``out``, a contiguous [R, I, O, S] tensor (it
    gives I, O and S).  ``idx`` / ``xrow`` (or None: X[p]) as in ttm_lookup_step; ``perm``: the contiguous int64 sample ids grouped
    by wrapped idx (``torch.sort(idx mod I, stable=True).indices``).  Nothing is read back: a bad index ORs ``flag`` and leaves
    ``out`` unwritten.  ``workspace``: uint8, at least ``ttm_lookup_grad_core_workspace_bytes``."""
    dt = dtype_code(X.dtype)
    assert X.dim() == 3 and X.is_contiguous() and dY.dtype == X.dtype and dY.device == X.device and dY.is_contiguous()
    rows_x, D, R = X.shape
    assert out.dim() == 4 and out.shape[0] == R and out.is_contiguous() and out.dtype == X.dtype and out.device == X.device
    I, O, S = out.shape[1], out.shape[2], out.shape[3]
    P, stride = _lookup_grad_indices("ttm_lookup_grad_core", idx, perm, xrow, flag, X.device)
    assert dY.numel() == P * D * O * S
    ws = workspace if workspace is not None else _workspace(ttm_lookup_grad_core_workspace_bytes(X.dtype, P, D, R, I, O, S), X.device)
    _call("ttr_ttm_lookup_grad_core", dt, P, rows_x, D, R, I, O, S, X.data_ptr(), _ptr(xrow), dY.data_ptr(), idx.data_ptr(), stride,
          perm.data_ptr(), out.data_ptr(), flag.data_ptr(), ws.data_ptr(), int(ws.numel()))
    return out


@_on_device
def ttm_lookup_grad_input(dY: torch.Tensor, G: torch.Tensor, idx: torch.Tensor, perm: torch.Tensor, flag: torch.Tensor,
                          out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ttr_ttm_lookup_grad_input: dX[p, dd, r] = sum_{o, s} dY[p, dd, o, s] G[r, idx[p], o, s] for dY (P D O S contiguous elements,
    read as [P, D, O, S]) and G [R, I, O, S] (passed with the strides it has, as to ttm_lookup_step) -> dX [P, D, R].  ``idx`` and
    ``perm`` as in ttm_lookup_grad_core.  ``out``: a contiguous tensor of P D R elements; ``workspace``: uint8, at least
    ``ttm_lookup_grad_input_workspace_bytes(P, I)``."""
    dt = dtype_code(G.dtype)
    assert G.dim() == 4 and dY.dtype == G.dtype and dY.device == G.device and dY.is_contiguous()
    R, I, O, S = G.shape
    P, stride = _lookup_grad_indices("ttm_lookup_grad_input", idx, perm, None, flag, G.device)
    assert dY.numel() % max(P * O * S, 1) == 0
    D = dY.numel() // (P * O * S) if P else 1
    if out is None:
        out = torch.empty((P, D, R), dtype=G.dtype, device=G.device)
    assert out.numel() == P * D * R and out.is_contiguous() and out.dtype == G.dtype and out.device == G.device
    if P == 0:
        return out
    ws = workspace if workspace is not None else _workspace(ttm_lookup_grad_input_workspace_bytes(P, I), G.device)
    _call("ttr_ttm_lookup_grad_input", dt, P, D, R, I, O, S, dY.data_ptr(), G.data_ptr(), _i64(G.stride()), idx.data_ptr(), stride,
          perm.data_ptr(), out.data_ptr(), flag.data_ptr(), ws.data_ptr(), int(ws.numel()))
    return out


@_on_device
def segment_sum(Y: torch.Tensor, seg: torch.Tensor, w: Optional[torch.Tensor] = None, perm: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ttr_segment_sum: out[b, :] = sum_{q = seg[b]}^{seg[b + 1] - 1} (w[src(q)] or 1) Y[src(q), :], src(q) = perm[q] (or q), for
    a contiguous Y [P, C], contiguous int64 device vectors ``seg`` [B + 1] (non-decreasing in 0 .. P) and ``perm`` [P], and ``w``
    [P] of Y's dtype -> out [B, C].  fp64 accumulation, one rounding, a fixed order."""
    dt = dtype_code(Y.dtype)
    assert Y.dim() == 2 and Y.is_contiguous() and Y.shape[1] >= 1
    P, C = Y.shape
    assert seg.dim() == 1 and seg.numel() >= 1 and seg.dtype == torch.int64 and seg.device == Y.device and seg.is_contiguous()
    B = seg.numel() - 1
    for t, ty in ((w, Y.dtype), (perm, torch.int64)):
        assert t is None or (tuple(t.shape) == (P,) and t.dtype == ty and t.device == Y.device and t.is_contiguous())
    if out is None:
        out = torch.empty((B, C), dtype=Y.dtype, device=Y.device)
    assert out.numel() == B * C and out.is_contiguous() and out.dtype == Y.dtype and out.device == Y.device
    if B == 0:
        return out
    _call("ttr_segment_sum", dt, B, P, C, _ptr(Y) if P else None, _ptr(w), _ptr(perm), seg.data_ptr(), out.data_ptr())
    return out


@_on_device
def env_half_apply(Phi: torch.Tensor, X: torch.Tensor, G: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ttr_env_half_apply: Phi [R, A, R'] (contiguous), X [R', J, S'] and G [A, I, J, A'] (both passed with the strides they have:
    a tt_transpose view or a rank-swapped view is read where it lies; the library refuses negative strides with
    NotImplementedError) -> H [R, I, A', S'] with H[r, i, c, s] = sum_{a, j} G[a, i, j, c] sum_b Phi[r, a, b] X[b, j, s].
    ValueError for anything but device tensors of one dtype whose extents fit.  ``out``: a contiguous tensor of R I A' S'
    elements that receives the result; fresh when None."""
    if Phi.dim() != 3 or X.dim() != 3 or G.dim() != 4 or not Phi.is_cuda:
        raise ValueError("env_half_apply: expected device tensors Phi [R, A, R'], X [R', J, S'] and G [A, I, J, A']")
    if not (X.dtype == Phi.dtype and G.dtype == Phi.dtype and X.device == Phi.device and G.device == Phi.device):
        raise ValueError("env_half_apply: the operands must have one dtype and lie on one device")
    dt = dtype_code(Phi.dtype)
    R, A, Rp = Phi.shape
    _, J, Sp = X.shape
    _, I, _, Ap = G.shape
    if X.shape[0] != Rp or G.shape[0] != A or G.shape[2] != J:
        raise ValueError("env_half_apply: Phi {}, X {} and G {} do not fit together".format(
            tuple(Phi.shape), tuple(X.shape), tuple(G.shape)))
    if not Phi.is_contiguous():
        raise ValueError("env_half_apply: Phi must be contiguous")
    shape = (R, I, Ap, Sp)
    if out is None:
        out = torch.empty(shape, dtype=Phi.dtype, device=Phi.device)
    if not (out.numel() == R * I * Ap * Sp and out.is_contiguous() and out.dtype == Phi.dtype and out.device == Phi.device):
        raise ValueError("env_half_apply: out must be a contiguous tensor of {} elements of the operands' dtype on their device".format(
            R * I * Ap * Sp))
    _call("ttr_env_half_apply", dt, R, A, Rp, J, Sp, I, Ap, Phi.data_ptr(), X.data_ptr(), _i64(X.stride()), G.data_ptr(),
          _i64(G.stride()), out.data_ptr())
    return out.view(shape)


def ritz_parts(dt: torch.dtype, n: int) -> int:
    """ttr_ritz_parts: the workgroups of the Gram launch for vectors of n elements, a function of n and the dtype alone."""
    parts = int(lib().ttr_ritz_parts(dtype_code(dt), int(n)))
    if parts < 0:
        _check(parts, "ttr_ritz_parts")
    return parts


def ritz_workspace_bytes(dt: torch.dtype, n: int) -> int:
    """ttr_ritz_workspace_bytes: the bytes of ``part``, 12 doubles per workgroup of the Gram launch."""
    wsb = int(lib().ttr_ritz_workspace_bytes(dtype_code(dt), int(n)))
    if wsb < 0:
        _check(wsb, "ttr_ritz_workspace_bytes")
    return wsb


def _ritz_vectors(who: str, X: torch.Tensor, others) -> int:
    if not (X.is_cuda and X.dim() == 1 and X.is_contiguous()):
        raise ValueError("{}: X must be a contiguous device vector".format(who))
    for v in others:
        if v is not None and not (v.shape == X.shape and v.dtype == X.dtype and v.device == X.device and v.is_contiguous()):
            raise ValueError("{}: the vectors must be contiguous, of X's length and dtype and on its device".format(who))
    return int(X.numel())


@_on_device
def ritz_gram(mode: int, X: torch.Tensor, AX: torch.Tensor, W: Optional[torch.Tensor] = None, AW: Optional[torch.Tensor] = None,
              P: Optional[torch.Tensor] = None, AP: Optional[torch.Tensor] = None, part: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ttr_ritz_gram: the fp64 partial sums [parts, 12] of S = V^T V and T = V^T A V, V = [X W P], for contiguous device vectors of
    one length and dtype (a view that starts off a 16-byte boundary takes the element loads, same bits).  ``mode`` is RITZ_INIT
    (X and AX only) or RITZ_STEP (P = AP = None: zeros, not read).  ``part``: a contiguous fp64 tensor that receives them."""
    n = _ritz_vectors("ritz_gram", X, (AX, W, AW, P, AP))
    dt = dtype_code(X.dtype)
    if part is None:
        part = torch.empty((ritz_parts(X.dtype, max(n, 1)), 12), dtype=torch.float64, device=X.device)
    if not (part.dtype == torch.float64 and part.is_contiguous() and part.device == X.device):
        raise ValueError("ritz_gram: part must be a contiguous fp64 tensor on the vectors' device")
    _call("ttr_ritz_gram", dt, int(mode), n, X.data_ptr(), AX.data_ptr(), _ptr(W), _ptr(AW), _ptr(P), _ptr(AP), part.data_ptr(),
          int(part.numel()) * 8)
    return part


@_on_device
def ritz_update(mode: int, which: int, first: int, rel: float, part: torch.Tensor, X: torch.Tensor, AX: torch.Tensor, W: torch.Tensor,
                AW: Optional[torch.Tensor], P: Optional[torch.Tensor], AP: Optional[torch.Tensor], state: torch.Tensor,
                sweep: torch.Tensor) -> None:
    """ttr_ritz_update, in place: finishes the sums of ``part`` (what ritz_gram returned for the same vectors), solves the 3 x 3
    pencil on the device and updates X, AX, W, P, AP; ``state`` (fp64[8]) is overwritten, ``sweep`` (fp64[4]) accumulated.
    Nothing is read back.  See include/ttround_hip.h for the step."""
    n = _ritz_vectors("ritz_update", X, (AX, W, AW, P, AP))
    dt = dtype_code(X.dtype)
    if not (part.dtype == torch.float64 and part.is_contiguous() and part.device == X.device
            and part.numel() == 12 * ritz_parts(X.dtype, max(n, 1))):
        raise ValueError("ritz_update: part must be the contiguous fp64 [parts, 12] tensor of ritz_gram for these vectors")
    for t, k in ((state, 8), (sweep, 4)):
        if not (t.dtype == torch.float64 and t.is_contiguous() and t.device == X.device and t.numel() == k):
            raise ValueError("ritz_update: state and sweep must be contiguous fp64 device tensors of 8 and 4 elements")
    _call("ttr_ritz_update", dt, int(mode), int(which), int(first), n, float(rel), part.data_ptr(), X.data_ptr(), AX.data_ptr(),
          W.data_ptr(), _ptr(AW), _ptr(P), _ptr(AP), state.data_ptr(), sweep.data_ptr())


def cg_parts(dt: torch.dtype, n: int) -> int:
    """ttr_cg_parts: the workgroups of each launch of a CG step on vectors of n elements, a function of n and the dtype alone."""
    parts = int(lib().ttr_cg_parts(dtype_code(dt), int(n)))
    if parts < 0:
        _check(parts, "ttr_cg_parts")
    return parts


def cg_workspace_bytes(dt: torch.dtype, n: int) -> int:
    """ttr_cg_workspace_bytes: the bytes of ``part``, two rows of ``cg_parts`` doubles."""
    wsb = int(lib().ttr_cg_workspace_bytes(dtype_code(dt), int(n)))
    if wsb < 0:
        _check(wsb, "ttr_cg_workspace_bytes")
    return wsb


def _cg_operands(who: str, vecs, part: torch.Tensor, state: Optional[torch.Tensor]) -> int:
    """The length of the contiguous device vectors ``vecs`` of one dtype; ``part`` and ``state`` are contiguous fp64 tensors on
    their device (the library checks the size of ``part``), ``state`` of 8 elements."""
    x = vecs[0]
    if not (x.is_cuda and x.dim() == 1 and x.is_contiguous()):
        raise ValueError("{}: the vectors must be contiguous device vectors".format(who))
    for v in vecs[1:]:
        if not (v.shape == x.shape and v.dtype == x.dtype and v.device == x.device and v.is_contiguous()):
            raise ValueError("{}: the vectors must be contiguous, of one length and dtype and on one device".format(who))
    for t, k in ((part, None), (state, 8)):
        if t is not None and not (t.dtype == torch.float64 and t.is_contiguous() and t.device == x.device
                                  and (k is None or t.numel() == k)):
            raise ValueError("{}: part and state must be contiguous fp64 tensors on the vectors' device, state of 8 elements".format(who))
    return int(x.numel())


@_on_device
def cg_dot(p: torch.Tensor, Bp: torch.Tensor, part: torch.Tensor) -> None:
    """ttr_cg_dot: row 0 of ``part`` (fp64 [2, cg_parts]) receives the workgroups' shares of p . Bp."""
    n = _cg_operands("cg_dot", (p, Bp), part, None)
    _call("ttr_cg_dot", dtype_code(p.dtype), n, p.data_ptr(), Bp.data_ptr(), part.data_ptr(), int(part.numel()) * 8)


@_on_device
def cg_update(step: int, p: torch.Tensor, Bp: torch.Tensor, v: torch.Tensor, r: torch.Tensor, part: torch.Tensor,
              state: torch.Tensor) -> None:
    """ttr_cg_update, in place: finishes p . Bp from row 0 of ``part``, forms alpha from ``state`` (fp64[8]) on the device,
    v += alpha p, r -= alpha Bp, and the shares of r . r go to row 1.  Nothing is read back.  See include/ttround_hip.h."""
    n = _cg_operands("cg_update", (p, Bp, v, r), part, state)
    _call("ttr_cg_update", dtype_code(p.dtype), int(step), n, p.data_ptr(), Bp.data_ptr(), v.data_ptr(), r.data_ptr(),
          part.data_ptr(), int(part.numel()) * 8, state.data_ptr())


@_on_device
def cg_direction(step: int, r: torch.Tensor, p: torch.Tensor, part: torch.Tensor, state: torch.Tensor) -> None:
    """ttr_cg_direction, in place: finishes r . r from row 1 of ``part``, forms beta, p = r + beta p, and stores the next rs in
    ``state``."""
    n = _cg_operands("cg_direction", (r, p), part, state)
    _call("ttr_cg_direction", dtype_code(p.dtype), int(step), n, r.data_ptr(), p.data_ptr(), part.data_ptr(), int(part.numel()) * 8,
          state.data_ptr())

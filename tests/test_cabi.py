"""The C-ABI shared library loads on a CPU-only box and exports every symbol that
include/ttround_hip.h declares (no compute calls: there is no GPU here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ttround_hip.h")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()  # hipcc cross-compiles gfx950 without a GPU
    return ctypes.CDLL(g.LIB)


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ttr_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported(lib):
    names = declared_functions()
    assert len(names) >= 12
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/ttround_hip.h but not exported"


def test_binding_matches_header(lib):
    from tntorch_amd import _hip

    assert sorted(_hip.EXPORTED_SYMBOLS) == declared_functions()


def _header_defines():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {n: int(v) for n, v in re.findall(r"^#define\s+(TTR_\w+)\s+\(?(-?\d+)\)?\s*$", src, flags=re.M)}


def test_parser_finds_every_declaration_once():
    """The binding's table is what its parser reads from the header: the names of ``declared_functions()``, one signature each."""
    from tntorch_amd import _hip

    sigs, defines = _hip._parse_header(open(HEADER).read())
    assert sorted(sigs) == declared_functions()
    assert sigs == _hip._SIGNATURES and _hip.EXPORTED_SYMBOLS == tuple(sigs)
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert len(re.findall(r"\bttr_[a-z0-9_]+\s*\(", src)) == len(sigs)   # no name is declared twice
    assert defines == _header_defines()


def test_parsed_signatures_pinned():
    """Written out by hand from the header, one entry per shape the parser has to handle: (void), a const char* result, an
    int64_t result, doubles, pointers to pointers, typed out-pointers, and the longest recent declaration."""
    from ctypes import c_char_p, c_double, c_int, c_int64, c_void_p

    from tntorch_amd import _hip

    i, q, d, p = c_int, c_int64, c_double, c_void_p
    pins = {
        "ttr_version": (i, []),
        "ttr_last_error": (c_char_p, []),
        "ttr_gemm_workspace_bytes": (q, [i, q, q, q, q]),
        "ttr_gemm_axpby": (i, [i, i, i, q, q, q, p, q, q, p, q, q, p, q, q, d, d, q, p, q, p]),
        "ttr_round_tt_workspace_bytes": (q, [i, q, p, p, q, i]),
        "ttr_round_tt": (i, [i, q, p, q, p, p, i, i, d, d, i, p, p, p, p, q, p]),
        "ttr_prof_collect": (i, [p, p]),
        "ttr_als_normal": (i, [i, q, q, q, p, q, p, q, p, p, p, p, p, p, p, p]),
    }
    for name, sig in pins.items():
        assert _hip._SIGNATURES[name] == sig, name


def test_constants_come_from_the_header():
    from tntorch_amd import _hip

    defines = _header_defines()
    assert len(defines) >= 48
    for name, value in defines.items():
        assert getattr(_hip, name[len("TTR_"):]) == value, name
    assert _hip.PROF_KINDS == ("gemm", "qr_factor", "qr_apply", "eigh", "misc", "rotgram", "project", "rowgram")
    assert len(_hip.PROF_KINDS) == defines["TTR_PROF_NKINDS"]


@pytest.mark.parametrize("text, quoted", [
    ("int ttr_foo(int dtype, float x);", "float x"),                       # a type outside the map
    ("int ttr_foo(struct ttr_shape s);", "struct ttr_shape s"),
    ("int ttr_foo(int dtype, const struct ttr_shape* s);", "const struct ttr_shape* s"),
    ("unsigned ttr_foo(void);", "unsigned"),
    ("int ttr_foo(int (*callback)(int), void* stream);", "int (*callback)(int)"),   # a ttr_foo( that is not a plain declaration
    ("int ttr_foo(int dtype, void* stream)\nint ttr_bar(void);", "ttr_foo(int dtype, void* stream)"),
    ("int ttr_foo();", "''"),
    ("#define TTR_FOO 1.5\n", "TTR_FOO 1.5"),
])
def test_parser_rejects_what_it_does_not_know(text, quoted):
    from tntorch_amd import _hip

    with pytest.raises(ValueError) as e:
        _hip._parse_header("#include <stdint.h>\nint ttr_ok(const void* const* p, int64_t* q, double v[3]);\n" + text)
    assert quoted in str(e.value)


def test_no_bare_knob_ids_or_status_codes_in_the_binding():
    """Knob ids and status codes are spelled by their header names in _hip.py, never as numbers."""
    src = open(os.path.join(ROOT, "tntorch_amd", "_hip.py")).read()
    src = re.sub(r"#[^\n]*", "", src)   # (comments quote the TTR_KNOBS syntax with numbers)
    knob_calls = re.findall(r"ttr_debug_set_knob\(\s*([^,)]*)", src)
    comparisons = re.findall(r"\bcode\s*[=!<>]=?\s*([^\s:)]+)", src)
    assert len(knob_calls) >= 4 and len(comparisons) >= 3
    for operand in knob_calls:
        assert not re.fullmatch(r"\(?-?\d+\)?", operand.strip()), f"ttr_debug_set_knob({operand}, ...)"
    for operand in comparisons:
        assert operand == "0" or not re.fullmatch(r"\(?-?\d+\)?", operand), f"code compared with {operand}"


def test_call_helper_only_launches_streamed_entries():
    """``_hip._call`` appends the current stream: every entry it is used for ends in ``void* stream`` in the header."""
    src = open(os.path.join(ROOT, "tntorch_amd", "_hip.py")).read()
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = set(re.findall(r'_call\("(ttr_\w+)"', src))
    assert len(names) >= 30
    for n in names:
        assert re.search(rf"\b{n}\s*\([^()]*\bvoid\*\s*stream\s*\)\s*;", header), n


def test_host_only_entry_points(lib):
    lib.ttr_version.restype = ctypes.c_int
    from tntorch_amd import _hip

    m = re.search(r"#define\s+TTR_ABI_VERSION\s+(\d+)", open(HEADER).read())
    assert m and lib.ttr_version() == int(m.group(1)) == _hip.ABI_VERSION  # header, library and binding agree
    lib.ttr_qr_max_cols.restype = ctypes.c_int
    assert lib.ttr_qr_max_cols(0) >= 64 and lib.ttr_qr_max_cols(1) >= 64
    lib.ttr_eigh_max_n_lds.restype = ctypes.c_int
    assert 64 <= lib.ttr_eigh_max_n_lds(1) <= lib.ttr_eigh_max_n_lds(0) <= 1024
    lib.ttr_qr_workspace_bytes.restype = ctypes.c_int64
    lib.ttr_qr_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]
    w1 = lib.ttr_qr_workspace_bytes(0, 4096, 64, 1)
    assert w1 >= 4096 * 64 * 4
    w8 = lib.ttr_qr_workspace_bytes(0, 4096, 64, 8)
    assert 8 * w1 - 8 * 64 * 4 * 4 <= w8 <= 8 * w1  # per-level tau arrays are padded to 64 elements per level, not per item
    assert lib.ttr_qr_workspace_bytes(1, 4096, 64, 1) == 2 * w1
    # argument validation happens before any HIP call
    lib.ttr_qr.restype = ctypes.c_int
    lib.ttr_last_error.restype = ctypes.c_char_p
    lib.ttr_norm.restype = ctypes.c_int
    lib.ttr_norm.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                             ctypes.c_void_p, ctypes.c_void_p]
    assert lib.ttr_norm(7, 1, 1, None, 0, None, None) == -1
    assert b"dtype" in lib.ttr_last_error()


def test_one_build_recipe():
    """csrc/Makefile is the manifest: it lists exactly the sources that exist, build() compiles exactly that list, and the
    eigensolver keeps its measured per-file flag."""
    import __graft_entry__ as g

    csrc = os.path.join(ROOT, "tntorch_amd", "csrc")
    text = open(os.path.join(csrc, "Makefile")).read().replace("\\\n", " ")
    src = re.search(r"^SRC\s*:=(.*)$", text, flags=re.M).group(1).split()
    assert sorted(src) == sorted(f for f in os.listdir(csrc) if f.endswith(".hip")) and len(set(src)) == len(src)
    assert g.SOURCES == src
    assert "-fno-slp-vectorize" in g.EXTRA_FLAGS["ttr_eigh.hip"]


def test_every_included_header_is_a_build_dependency():
    """Every quoted #include of the library's sources and headers names a file of the Makefile's HDR, which is also the list
    ``build()`` checks for staleness: a header left out would mean silently stale objects."""
    import __graft_entry__ as g

    csrc = os.path.join(ROOT, "tntorch_amd", "csrc")
    text = open(os.path.join(csrc, "Makefile")).read().replace("\\\n", " ")
    hdr = [os.path.normpath(os.path.join(csrc, h)) for h in re.search(r"^HDR\s*:=(.*)$", text, flags=re.M).group(1).split()]
    assert g.HEADERS == hdr and len(set(hdr)) == len(hdr) and all(os.path.isfile(h) for h in hdr)
    files = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".h"))]
    files += [os.path.join(csrc, "detail", f) for f in os.listdir(os.path.join(csrc, "detail")) if f.endswith(".h")]
    seen = set()
    for path in files:
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), flags=re.M):
            target = os.path.normpath(os.path.join(os.path.dirname(path), inc))
            assert target in hdr, f"{os.path.relpath(path, ROOT)} includes {inc}, which HDR does not list"
            seen.add(target)
    assert seen == set(hdr)   # and HDR lists nothing that no file includes


def test_no_silent_fallback_for_device_tensors(monkeypatch):
    """A CUDA tensor must never be routed to the host mirror; missing library => RuntimeError."""
    import torch

    from tntorch_amd import _dispatch, _hip, _hostops

    assert _dispatch.ops_for(torch.zeros(2)) is _hostops
    monkeypatch.setattr(_hip, "LIB_PATH", "/nonexistent/libttround_hip.so")
    monkeypatch.setattr(_hip, "_lib", None)

    class FakeDev:
        type = "cuda"

    class FakeT:
        device = FakeDev()
        dtype = torch.float32

    with pytest.raises(RuntimeError, match="not found"):
        _dispatch.ops_for(FakeT())


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "tntorch_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                txt = open(os.path.join(dp, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt, f

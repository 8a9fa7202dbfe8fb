"""CPU-only: recalgorithm_amd/_abi.py, the reader that derives the ctypes bindings from include/recalgo.h and
include/recalgo_host.h — known answers on declarations written here, the host compiler as the referee of the struct
layouts, every re-exported constant against its #define, and the errcheck of the kernel-launching entries."""
import ctypes
import os
import re
import shutil
import subprocess
from ctypes import (c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_ubyte, c_uint, c_uint32, c_uint64, c_void_p)

import pytest

from recalgorithm_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
TEN_STRUCTS = {"recalgo_live_t", "recalgo_colsum_t", "recalgo_dense_split_t", "recalgo_dropout_t", "recalgo_adam_arena_t",
               "recalgo_scatter_source_t", "recalgo_scatter_companion_t", "recalgo_plan_scan_t", "recalgo_deferred_adam_t",
               "recalgo_lookup_job_t"}

KNOWN = """
/* a comment with a declaration inside: int recalgo_not_this(int a); */
#ifndef RECALGO_T_H_
#define RECALGO_T_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef void* recalgo_stream_t; /* hipStream_t */
#define RECALGO_DEC 16
#define RECALGO_HEX 0x100
#define RECALGO_NEG (-1)      /* trailing comment */
#define RECALGO_ABI_VERSION 7
int recalgo_version(void);
const char* recalgo_name(void);
void recalgo_close(void* h);
void* recalgo_open(const char* path, const char* const* keys, unsigned flags, unsigned int more);
uint32_t recalgo_crc(const void* data, uint64_t n, uint32_t seed);
int64_t recalgo_bytes(int32_t a, int64_t b, float c, double d, unsigned char e);
int recalgo_parts_fwd(const float* const* x_parts, const int* widths, int n,
                      float* out, recalgo_stream_t stream);
int recalgo_plan(void* ws, recalgo_stream_t stream, int after_the_stream);
int64_t recalgo_rows(int B, recalgo_stream_t stream);
typedef struct {
    float* w; float* m; float* v;   /* [rows, K] */
    int n_ex, F;
    unsigned seed, call;
    const char* name;
    const int64_t* step;
    unsigned char flag;
    double rate;
    recalgo_stream_t stream;
} recalgo_mixed_t;
typedef struct recalgo_tagged { uint32_t a, b; int64_t c; } recalgo_tagged_t;
#ifdef __cplusplus
}
#endif
#endif /* RECALGO_T_H_ */
"""


def test_known_answers_functions():
    abi = _abi.parse(KNOWN)
    assert abi.functions == {
        "recalgo_version": (c_int, []),
        "recalgo_name": (c_char_p, []),
        "recalgo_close": (None, [c_void_p]),
        "recalgo_open": (c_void_p, [c_char_p, c_void_p, c_uint, c_uint]),
        "recalgo_crc": (c_uint32, [c_void_p, c_uint64, c_uint32]),
        "recalgo_bytes": (c_int64, [c_int32, c_int64, c_float, c_double, c_ubyte]),
        "recalgo_parts_fwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
        "recalgo_plan": (c_int, [c_void_p, c_void_p, c_int]),
        "recalgo_rows": (c_int64, [c_int, c_void_p]),
    }
    assert list(abi.functions)[:3] == ["recalgo_version", "recalgo_name", "recalgo_close"]        # header order
    # hipError_t by contract: returns int AND the stream is the last parameter
    assert abi.launches == ["recalgo_parts_fwd"]


def test_known_answers_structs_and_constants():
    abi = _abi.parse(KNOWN)
    assert list(abi.structs) == ["recalgo_mixed_t", "recalgo_tagged_t"]
    mixed = abi.structs["recalgo_mixed_t"]
    assert issubclass(mixed, ctypes.Structure)
    assert mixed._fields_ == [("w", c_void_p), ("m", c_void_p), ("v", c_void_p), ("n_ex", c_int), ("F", c_int), ("seed", c_uint),
                              ("call", c_uint), ("name", c_char_p), ("step", c_void_p), ("flag", c_ubyte), ("rate", c_double),
                              ("stream", c_void_p)]
    assert abi.structs["recalgo_tagged_t"]._fields_ == [("a", c_uint32), ("b", c_uint32), ("c", c_int64)]
    assert mixed(None, None, None, 3, 4).F == 4                                                    # positional, header order
    assert abi.constants == {"RECALGO_DEC": 16, "RECALGO_HEX": 256, "RECALGO_NEG": -1, "RECALGO_ABI_VERSION": 7}


def test_declaration_hash_known_answers():
    """what a version covers: the declarations, not the comments, the layout of the text or the version's own number"""
    h = _abi.declaration_hash("recalgo_t.h", text=KNOWN)
    assert h == "402ecdeb3dab77280ac0a3175cf20cddd380f112e35b70f1cbd554fe2c208d84"
    same = [KNOWN.replace("/* hipStream_t */", "/* a stream;\n int recalgo_x(int a); */"),
            KNOWN.replace("void* recalgo_open(const char* path, ", "void*   recalgo_open(const char* path,\n\t"),
            KNOWN.replace("#define RECALGO_ABI_VERSION 7", "#define RECALGO_ABI_VERSION 12"),
            "\n\n" + KNOWN + "  \n"]
    assert [_abi.declaration_hash("recalgo_t.h", text=t) for t in same] == [h] * 4 and len(set(same + [KNOWN])) == 5
    other = [KNOWN.replace("uint64_t n, uint32_t seed", "uint32_t n, uint32_t seed"),               # one parameter's type
             KNOWN.replace("int32_t a, int64_t b,", "int64_t b, int32_t a,"),                          # two parameters' order
             KNOWN.replace("#define RECALGO_DEC 16", "#define RECALGO_DEC 17"),                       # a constant that is no version
             KNOWN.replace("int n_ex, F;", "int F, n_ex;")]                                            # a struct's field order
    hashes = [_abi.declaration_hash("recalgo_t.h", text=t) for t in other]
    assert h not in hashes and len(set(hashes)) == 4
    # a keyed header's version define goes by the same rule (the whole line: name and number)
    keyed = KNOWN.replace("RECALGO_ABI_VERSION 7", "RECALGO_T9_ABI_VERSION 8")
    assert keyed != KNOWN and _abi.declaration_hash("recalgo_t.h", text=keyed) == h


@pytest.mark.parametrize("text, found", [
    ("int recalgo_abi_version(void);", r"found \[\] and \['recalgo_abi_version'\]"),                                # no define
    ("#define RECALGO_ABI_VERSION 1\nint recalgo_f(void);", r"found \['RECALGO_ABI_VERSION'\] and \[\]"),           # no function
    ("#define RECALGO_X_ABI_VERSION 1\nint recalgo_abi_version(void);", "found"),                                  # another key's
    ("#define RECALGO_ABI_VERSION 1\n#define RECALGO_X_ABI_VERSION 1\nint recalgo_abi_version(void);", "found"),    # two defines
    ("#define RECALGO_X_ABI_VERSION 1\nint recalgo_x_abi_version(void);\nint recalgo_abi_version(void);", "found"),   # two functions
])
def test_a_table_header_without_one_version_pair_raises_and_names_the_header(text, found, monkeypatch):
    monkeypatch.setattr(_abi, "read", lambda header: _abi.parse(text, header))
    with pytest.raises(_lib.RecalgoError, match=r"^include/recalgo_t\.h: .*" + found):
        _lib._versioned("recalgo_t.h")
    assert not hasattr(_abi.parse(text), "version")          # parse itself takes text without a version pair as it is


def test_a_table_header_with_its_version_pair():
    assert _lib.HEADERS["recalgo.h"].version == 5 and _lib.HEADERS["recalgo.h"].version_query == "recalgo_abi_version"
    assert [(h, a.label) for h, a in _lib.HEADERS.items()][:4] == [
        ("recalgo.h", "ABI"), ("recalgo_cgc.h", "CGC ABI"), ("recalgo_wide.h", "WIDE ABI"), ("recalgo_bst.h", "BST ABI")]


@pytest.mark.parametrize("bad, line", [
    ("int recalgo_f(long n);", 1),                                        # a type outside the table: parameter,
    ("\nlong recalgo_f(int n);", 2),                                      # return type,
    ("\n\ntypedef struct { long n; } recalgo_s_t;", 3),                   # struct field
    ("int recalgo_f(int);", 1),                                           # unnamed parameter
    ("int recalgo_f();", 1),                                              # K&R parameter list
    ("int recalgo_a(void);\nint recalgo_f(int (*cb)(int));", 2),          # function pointer
    ("typedef struct { int a[4]; } recalgo_s_t;", 1),                     # array field
    ("typedef struct { int *a, *b; } recalgo_s_t;", 1),                   # pointer declarators after a comma
    ("typedef int recalgo_int_t;", 1),                                    # a typedef other than the stream's
    ("int recalgo_a(void);\n#define RECALGO_RATE 0.5", 2),                # a non-integer define
    ("#pragma once", 1),
    ("int recalgo_f(int n)", 1),                                          # no terminator
])
def test_what_the_reader_does_not_know_raises_and_names_the_line(bad, line):
    with pytest.raises(_lib.RecalgoError, match=rf"hdr\.h:{line}:"):
        _abi.parse(bad, "hdr.h")


def test_missing_header_raises_with_the_path():
    with pytest.raises(_lib.RecalgoError, match=re.escape(os.path.join(INCLUDE, "recalgo_nope.h"))):
        _abi.read("recalgo_nope.h")


def _c_structs(header):
    """-> {struct: [field names]} by a parse of its own: the last identifier of every declarator between the braces"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(recalgo_\w+_t)\s*;", src, flags=re.S):
        out[name] = [re.search(r"(\w+)\s*$", d).group(1) for stmt in body.split(";") if stmt.strip() for d in stmt.split(",")]
    return out


def test_struct_layouts_agree_with_the_host_compiler(tmp_path):
    """A C++ program that includes recalgo.h prints sizeof and every offsetof of every recalgo_*_t; ctypes must lay the
    derived classes out the same way."""
    structs = _c_structs("recalgo.h")
    assert TEN_STRUCTS <= set(structs)
    assert set(structs) == set(_lib.STRUCTS)
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "recalgo.h"', "int main() {"]
    for name, fields in structs.items():
        lines.append(f'  std::printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'  std::printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f in fields]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    cxx = shutil.which("g++") or "g++"                        # the host compiler of build.build_host
    subprocess.run([cxx, "-std=c++17", f"-I{INCLUDE}", str(src), "-o", str(exe)], check=True)
    compiled = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    derived = {}
    for name, cls in _lib.STRUCTS.items():
        assert [f for f, _ in cls._fields_] == structs[name], name
        derived[name] = str(ctypes.sizeof(cls))
        derived.update((f"{name}.{f}", str(getattr(cls, f).offset)) for f, _ in cls._fields_)
    assert derived == compiled
    assert [int(compiled[n]) for n in ("recalgo_live_t", "recalgo_dropout_t", "recalgo_dense_split_t", "recalgo_colsum_t",
                                       "recalgo_adam_arena_t", "recalgo_plan_scan_t", "recalgo_scatter_source_t",
                                       "recalgo_deferred_adam_t", "recalgo_scatter_companion_t", "recalgo_lookup_job_t")] \
        == [32, 32, 40, 40, 64, 32, 88, 56, 56, 72]


def _defines(header):
    """-> {name: int} of the integer #defines, by a parse of its own"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
    return {n: int(v, 0) for n, v in re.findall(r"^#define\s+(RECALGO_\w+)[ \t]+\(?(-?\w+)\)?[ \t]*$", src, flags=re.M)}


def test_every_constant_in_use_equals_the_header():
    from recalgorithm_amd import ops, sparse
    from recalgorithm_amd.io import native
    d = _defines("recalgo.h")
    assert d == _lib.CONSTANTS and len(d) >= 19
    assert _lib.ABI_VERSION == d["RECALGO_ABI_VERSION"] == 5
    assert native.ABI.constants == _defines("recalgo_host.h") == {"RECALGO_HOST_ABI_VERSION": 1}
    in_use = {
        "RECALGO_ACT_NONE": ops._ACT_NONE, "RECALGO_ACT_PRELU": ops._ACT["prelu"], "RECALGO_ACT_DICE": ops._ACT["dice"],
        "RECALGO_BILINEAR_ALL": ops.BILINEAR_TYPES["all"], "RECALGO_BILINEAR_EACH": ops.BILINEAR_TYPES["each"],
        "RECALGO_BILINEAR_INTERACTION": ops.BILINEAR_TYPES["interaction"],
        "RECALGO_PNN_IPNN": ops.PNN_METHODS["IPNN"], "RECALGO_PNN_OPNN": ops.PNN_METHODS["OPNN"],
        "RECALGO_GATE_MIX_MAX": ops.GATE_MIX_MAX,
        "RECALGO_SCATTER_GRAD": sparse.MODE_GRAD, "RECALGO_SCATTER_ADAM": sparse.MODE_ADAM,
        "RECALGO_SCATTER_LAZY_ADAM": sparse.MODE_LAZY_ADAM, "RECALGO_SCATTER_PRESCANNED": sparse.MODE_PRESCANNED,
        "RECALGO_PREPARE_COUNT": sparse.PREPARE_COUNT, "RECALGO_PREPARE_SWEEP": sparse.PREPARE_SWEEP,
        "RECALGO_PREPARE_CATCHUP": sparse.PREPARE_CATCHUP,
        "RECALGO_SCATTER_MAX_SOURCES": sparse.MAX_SOURCES, "RECALGO_LR_RING": sparse.LR_RING,
        "RECALGO_ABI_VERSION": _lib.ABI_VERSION,
    }
    assert in_use == d                                       # every #define of the header is re-exported, each with its value
    assert len(ops._ACT) == 2 and len(ops.BILINEAR_TYPES) == 3 and len(ops.PNN_METHODS) == 2
    assert (d["RECALGO_ACT_NONE"], d["RECALGO_SCATTER_PRESCANNED"], d["RECALGO_LR_RING"]) == (-1, 0x100, 1024)


def test_the_struct_names_the_wrappers_use_are_the_derived_classes():
    from recalgorithm_amd import ops, sparse
    S = _lib.STRUCTS
    assert (ops._Live, ops._ColSum, ops._DenseSplit, ops._CDrop, ops._AdamArena) == (
        S["recalgo_live_t"], S["recalgo_colsum_t"], S["recalgo_dense_split_t"], S["recalgo_dropout_t"], S["recalgo_adam_arena_t"])
    assert (sparse._CSource, sparse._CCompanion, sparse._CPlanScan, sparse._CDeferred, sparse._CLookupJob) == (
        S["recalgo_scatter_source_t"], S["recalgo_scatter_companion_t"], S["recalgo_plan_scan_t"], S["recalgo_deferred_adam_t"],
        S["recalgo_lookup_job_t"])


def test_errcheck_raises_on_an_error_code_and_names_the_entry():
    ec = _lib.launch_errcheck("recalgo_stub_fwd")
    assert ec(0, None, ()) == 0
    with pytest.raises(_lib.RecalgoError, match=r"^recalgo_stub_fwd failed with hipError_t=1$"):
        ec(1, None, ())

    # through ctypes, on a stub that is no GPU entry: abs(-3) is the "error code"
    libc = ctypes.CDLL(None)
    stub = libc.abs
    stub.restype, stub.argtypes, stub.errcheck = c_int, [c_int], _lib.launch_errcheck("recalgo_stub_bwd")
    assert stub(0) == 0
    with pytest.raises(_lib.RecalgoError, match="recalgo_stub_bwd failed with hipError_t=3"):
        stub(-3)


def test_errcheck_is_attached_to_exactly_the_stream_taking_int_entries():
    from recalgorithm_amd import build
    build.build(verbose=False)
    lib = _lib.load()
    # the rule, from the header's text by a parse of its own: `int name(..., recalgo_stream_t stream);`
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "recalgo.h")).read(), flags=re.S)
    want = set(re.findall(r"\bint\s+(recalgo_\w+)\s*\([^)]*\brecalgo_stream_t\s+\w+\s*\)\s*;", src))
    every = set(re.findall(r"\b(recalgo_[a-z0-9_]+)\s*\(", src))
    assert len(want) == 77 and every == set(_lib.SIGNATURES)
    attached = {n for n in _lib.SIGNATURES if getattr(lib, n).errcheck is not None}
    assert attached == want == set(_lib.ABI.launches)
    for n in ("recalgo_abi_version", "recalgo_target_arch", "recalgo_scatter_plan_scan", "recalgo_gate_mix_supported",
              "recalgo_dense_bwd_rider_supported", "recalgo_cross_bwd_workspace_bytes", "recalgo_batchnorm_partial_rows"):
        assert n in _lib.SIGNATURES and n not in attached
    for n in every - want:                                   # the queries: no stream anywhere in their parameters
        assert "recalgo_stream_t" not in re.search(r"\b" + n + r"\s*\(([^)]*)\)", src).group(1), n

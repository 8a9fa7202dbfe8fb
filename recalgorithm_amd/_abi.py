"""Reader of the C-ABI headers (include/recalgo.h, include/recalgo_host.h): the ctypes bindings are DERIVED from the
declarations the HIP and C++ sources compile against, so the header is the only statement of the ABI.

    abi = read("recalgo.h")
    abi.functions   name -> (restype, argtypes), in header order
    abi.launches    the functions that return int and take a recalgo_stream_t last: by the header's contract their return
                    value is a hipError_t
    abi.structs     name -> ctypes.Structure subclass of each `typedef struct { .. } recalgo_*_t;`, fields in header order
    abi.constants   name -> int of each `#define RECALGO_* <integer>` (the ABI version among them)

    declaration_hash("recalgo.h")   what an ABI version covers: the sha256 of the header's declarations
    read_record("recalgo.h")        version -> that hash, as include/recalgo.abi recorded it when the version was set

One type rule serves parameters, return types and struct fields (`ctype_of`).  The reader knows exactly the constructs the
two headers use; anything else raises RecalgoError naming the line — it never skips a declaration.
"""
from __future__ import annotations

import ctypes
import hashlib
import os
import re
from types import SimpleNamespace

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


class RecalgoError(RuntimeError):
    pass


_SCALARS = {
    "int": ctypes.c_int, "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint, "unsigned char": ctypes.c_ubyte,
    "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64,
    "float": ctypes.c_float, "double": ctypes.c_double,
}
_DEFINE = re.compile(r"#\s*define\s+(RECALGO_\w+)\s+\(?\s*(-?\s*(?:0[xX][0-9a-fA-F]+|\d+))\s*\)?$")
_IGNORED = re.compile(r"#\s*(ifndef\s+\w+|define\s+\w+_H_|include\s*<stdint\.h>|endif)$")    # include guard, <stdint.h>
_STRUCT = re.compile(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(recalgo_\w+_t)\s*;")
_STREAM = re.compile(r"typedef\s+void\s*\*\s*recalgo_stream_t\s*;")
_FUNCTION = re.compile(r"([\w\s\*]+?)\b(recalgo_\w+)\s*\(([^(){};]*)\)\s*;")
_SPACE = re.compile(r"\s*")


def ctype_of(ctype: str, where: str = "?"):
    """The ctypes type of a C type (no declarator name): single-level char* -> c_char_p, any other pointer and
    recalgo_stream_t -> c_void_p, the fixed-width and plain scalars by name."""
    t = " ".join(w for w in ctype.replace("*", " * ").split() if w != "const")
    if t == "char *":
        return ctypes.c_char_p
    if t.endswith("*") or t == "recalgo_stream_t":
        return ctypes.c_void_p
    if t not in _SCALARS:
        raise RecalgoError(f"{where}: unknown C type `{ctype.strip()}`")
    return _SCALARS[t]


def _declarator(decl: str, where: str):
    """`const float* const* x_parts` -> (`const float* const*`, `x_parts`)"""
    m = re.fullmatch(r"\s*(.*[\s\*])(\w+)\s*", decl, flags=re.S)
    if not m:
        raise RecalgoError(f"{where}: cannot parse the declaration `{decl.strip()}`")
    return m.group(1), m.group(2)


def _fields(body: str, where: str):
    """`float* w; float* m; int n_ex, F;` -> [(name, ctype)]: the declarators after a comma share the first one's type"""
    out = []
    for stmt in filter(str.strip, body.split(";")):
        first, *more = stmt.split(",")
        ctype, name = _declarator(first, where)
        t = ctype_of(ctype, where)
        for n in [name] + [s.strip() for s in more]:
            if not re.fullmatch(r"\w+", n):
                raise RecalgoError(f"{where}: cannot parse the declarator `{n}` of `{stmt.strip()}`")
            out.append((n, t))
    return out


def parse(text: str, origin: str = "<string>") -> SimpleNamespace:
    blank = lambda m: "\n" * m.group().count("\n")      # (what is removed keeps its line breaks: errors name the header's line)
    text = re.sub(r"/\*.*?\*/", blank, text, flags=re.S)
    text = re.sub(r"#\s*ifdef\s+__cplusplus\b.*?#\s*endif", blank, text, flags=re.S)    # extern "C" { .. }
    abi = SimpleNamespace(functions={}, launches=[], structs={}, constants={})
    lines = text.split("\n")
    for i, ln in enumerate(lines):
        if not ln.lstrip().startswith("#"):
            continue
        m = _DEFINE.match(ln.strip())
        if m:
            abi.constants[m.group(1)] = int(m.group(2).replace(" ", ""), 0)
        elif not _IGNORED.match(ln.strip()):
            raise RecalgoError(f"{origin}:{i + 1}: cannot parse `{ln.strip()}`")
        lines[i] = ""
    text, pos = "\n".join(lines), 0
    while True:
        pos = _SPACE.match(text, pos).end()
        if pos == len(text):
            return abi
        where = f"{origin}:{text.count(chr(10), 0, pos) + 1}"
        m = _STRUCT.match(text, pos) or _STREAM.match(text, pos) or _FUNCTION.match(text, pos)
        if not m:
            raise RecalgoError(f"{where}: cannot parse the declaration `{text[pos:pos + 60].split(chr(10))[0]}`")
        if m.re is _STRUCT:
            abi.structs[m.group(2)] = type(m.group(2), (ctypes.Structure,), {"_fields_": _fields(m.group(1), where)})
        elif m.re is _FUNCTION:
            ret, name, params = m.group(1), m.group(2), m.group(3).strip()
            params = [] if params == "void" else [_declarator(p, where)[0] for p in params.split(",")]
            res = None if ret.split() == ["void"] else ctype_of(ret, where)
            abi.functions[name] = (res, [ctype_of(p, where) for p in params])
            if res is ctypes.c_int and params and params[-1].split() == ["recalgo_stream_t"]:
                abi.launches.append(name)
        pos = m.end()


def _text(header: str) -> str:
    path = os.path.join(INCLUDE, header)
    if not os.path.exists(path):
        raise RecalgoError(f"{path} not found: the ctypes binding is derived from it")
    with open(path) as f:
        return f.read()


def read(header: str) -> SimpleNamespace:
    return parse(_text(header), os.path.join(INCLUDE, header))


def declaration_hash(header: str, text: str = None) -> str:
    """sha256 over the declarations of include/<header> (or of `text`, a header's content): comments, the header's
    `#define RECALGO_[<KEY>_]ABI_VERSION <n>` and runs of white space removed.  What this covers is what a version stands for:
    the declarations may not change while the number stays (include/<stem>.abi, tests/test_abi.py)."""
    src = re.sub(r"/\*.*?\*/", "", _text(header) if text is None else text, flags=re.S)
    src = re.sub(r"#define RECALGO_(?:[A-Z0-9]+_)?ABI_VERSION \d+", "", src)
    return hashlib.sha256(re.sub(r"\s+", " ", src).strip().encode()).hexdigest()


def record_path(header: str) -> str:
    return os.path.join(INCLUDE, os.path.splitext(header)[0] + ".abi")


def read_record(header: str) -> dict:
    """include/<stem>.abi -> {version: declaration hash}: one `version sha256` line per version, `#` starts a comment line"""
    with open(record_path(header)) as f:
        return {int(v): h for v, h in (ln.split() for ln in f if ln.strip() and not ln.startswith("#"))}

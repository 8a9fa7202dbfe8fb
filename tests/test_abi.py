"""CPU-only: the C-ABI shared library builds, loads and exports exactly what the headers of _lib.HEADERS declare; the ctypes
binding covers every declaration of every header, and each header's version moves with its declarations.  Every check runs
once per header (the test id is the header's file name): a new header is checked by being in the table.  What a feature
expects of its own header, literally, is in that feature's host test.  No compute calls (no GPU here)."""
import ctypes
import os
import re

import pytest

from recalgorithm_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = list(_lib.HEADERS)
per_header = pytest.mark.parametrize("header", HEADERS, ids=HEADERS)


def source(header):
    """the header's text without comments (every parse below is this file's own, not _abi's)"""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)


def declared_functions(header):
    return sorted(set(re.findall(r"\b(recalgo_[a-z0-9_]+)\s*\(", source(header))))


def version_define(header):
    """(define's name, number, label in error messages) of the header's one version define, from its text"""
    (name, key, number), = re.findall(r"#define (RECALGO_(?:([A-Z0-9]+)_)?ABI_VERSION) (\d+)", source(header))
    return name, int(number), (key + " ABI" if key else "ABI")


@pytest.fixture(scope="module")
def lib_path():
    from recalgorithm_amd import build
    return build.build(verbose=False)


def test_the_table_lists_the_headers_in_order():
    assert HEADERS[:4] == ["recalgo.h", "recalgo_cgc.h", "recalgo_wide.h", "recalgo_bst.h"]
    assert _lib.ABI is _lib.HEADERS["recalgo.h"] and _lib.SIGNATURES is _lib.ABI.functions and _lib.STRUCTS is _lib.ABI.structs
    assert _lib.CONSTANTS is _lib.HEADERS["recalgo.h"].constants and _lib.ABI_VERSION == _lib.ABI.version


@per_header
def test_header_declares_functions(header):
    fns = declared_functions(header)
    assert fns and _lib.HEADERS[header].version_query in fns
    if header == "recalgo.h":
        assert "recalgo_embedding_gather_fwd" in fns and "recalgo_cross_fwd" in fns
        assert len(fns) >= 20


@per_header
def test_library_exports_every_declared_symbol(header, lib_path):
    import torch  # noqa: F401  maps the HIP runtime first
    lib = ctypes.CDLL(lib_path)
    missing = [f for f in declared_functions(header) if not hasattr(lib, f)]
    assert not missing, f"declared in {header} but not exported: {missing}"


@per_header
def test_ctypes_binding_matches_header(header, lib_path):
    abi = _lib.HEADERS[header]
    declared = set(declared_functions(header))
    bound = set(abi.functions)
    assert declared == bound, f"header-only: {declared - bound}; binding-only: {bound - declared}"
    lib = _lib.load()
    define, number, label = version_define(header)
    assert getattr(lib, abi.version_query)() == abi.version == number == abi.constants[define]
    assert abi.version_query == define.lower() and abi.label == label
    assert lib.recalgo_target_arch() == b"gfx950"


@per_header
def test_loaded_functions_carry_the_table(header, lib_path):
    abi = _lib.HEADERS[header]
    lib = _lib.load()
    assert set(abi.launches) <= set(abi.functions)
    for name, (res, args) in abi.functions.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
        assert (fn.errcheck is not None) == (name in abi.launches), name


@per_header
def test_declarations_do_not_change_without_a_version_bump(header):
    """include/<stem>.abi: one `version sha256` line per ABI version.  A stale librecalgo_hip.so with re-ordered
    arguments corrupts calls silently; _lib.load() catches it only if the version moved with the declarations."""
    define, version, _ = version_define(header)
    record = "include/" + os.path.splitext(header)[0] + ".abi"
    recorded = _abi.read_record(header)
    h = _abi.declaration_hash(header)
    assert version == max(recorded), f"{header} is at version {version}, {record} ends at {max(recorded)}"
    assert recorded[version] == h, (
        f"the declarations of include/{header} changed (sha256 {h}) but {define} is still {version}: bump it in "
        f"{header} and append `<version> {h}` to {record} (python scripts/abi_record.py {header})")
    assert len(set(recorded.values())) == len(recorded), "two ABI versions with identical declarations"
    # the reader of the record, against a parse of this file's own
    lines = [ln.split() for ln in open(os.path.join(ROOT, record)) if ln.strip() and not ln.startswith("#")]
    assert recorded == {int(v): sha for v, sha in lines} and len(lines) == len(recorded)


@per_header
def test_stale_version_fails_loudly(header, lib_path, monkeypatch):
    """a library of another version of ANY header is refused: the version the binding expects is read when load() runs"""
    abi = _lib.HEADERS[header]
    _, version, label = version_define(header)
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(abi, "version", version + 1)
    with pytest.raises(_lib.RecalgoError, match=re.escape(
            f"{_lib.LIB_PATH}: {label} version {version}, this binding expects {version + 1} "
            "(a stale build: python -m recalgorithm_amd.build)") + "$"):
        _lib.load()


@per_header
def test_header_arg_counts_match_binding(header):
    src = source(header)
    for name, (_, args) in _lib.HEADERS[header].functions.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src)
        assert m, name
        params = [p for p in m.group(1).split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == len(args), f"{name}: header has {len(params)} params, binding {len(args)}"


@per_header
def test_header_arg_types_match_binding(header):
    """Every parameter and return type of the header against the ctypes signature (int vs int64_t vs float vs
    pointer): a wrong width here silently corrupts arguments at call time."""
    from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_uint, c_uint64, c_void_p
    src = source(header)

    def ctype_of(decl):
        decl = decl.strip()
        if "*" in decl or decl.startswith("recalgo_stream_t"):
            return c_void_p
        base = decl.rsplit(" ", 1)[0].replace("const ", "").strip()
        return {"int": c_int, "int64_t": c_int64, "uint64_t": c_uint64, "float": c_float, "double": c_double, "unsigned": c_uint,
                "unsigned int": c_uint}[base]

    for name, (res, args) in _lib.HEADERS[header].functions.items():
        m = re.search(r"([A-Za-z_0-9 \*]+?)\b" + name + r"\s*\(([^)]*)\)", src)
        assert m, name
        ret = m.group(1).strip()
        want_res = c_char_p if "char" in ret else {"int": c_int, "int64_t": c_int64}[ret.replace("const ", "")]
        assert res is want_res, f"{name}: returns {ret}, binding {res}"
        params = [p for p in m.group(2).split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == len(args), name
        for i, (decl, bound) in enumerate(zip(params, args)):
            assert ctype_of(decl) is bound, f"{name} arg {i} `{decl.strip()}`: binding {bound.__name__}"


@per_header
def test_header_is_self_contained(header):
    """the reader takes each header as it is; every header but the first repeats the stream typedef instead of including
    recalgo.h, so a caller may include it alone"""
    text = open(os.path.join(ROOT, "include", header)).read()
    assert "typedef void* recalgo_stream_t;" in text
    if header != "recalgo.h":
        assert '#include "recalgo.h"' not in text
    assert _abi.read(header).constants == _lib.HEADERS[header].constants


def test_the_headers_share_no_name():
    """every header against every other one, whichever came first"""
    prefixes = {}
    for i, a in enumerate(HEADERS):
        for b in HEADERS[i + 1:]:
            assert not set(_lib.HEADERS[a].functions) & set(_lib.HEADERS[b].functions), (a, b)
            assert not set(_lib.HEADERS[a].constants) & set(_lib.HEADERS[b].constants), (a, b)
        define = version_define(a)[0]
        if a == "recalgo.h":
            assert define == "RECALGO_ABI_VERSION"
        else:
            prefixes[a] = define[:-len("ABI_VERSION")]                 # RECALGO_<KEY>_
            assert prefixes[a] != "RECALGO_" and [k for k in _lib.HEADERS[a].constants if not k.startswith(prefixes[a])] == [], a
    assert len(set(prefixes.values())) == len(HEADERS) - 1
    assert not [k for k in _lib.CONSTANTS if k.startswith(tuple(prefixes.values()))]
    assert _lib.CONSTANTS is _lib.HEADERS["recalgo.h"].constants


def test_object_code_is_gfx950(lib_path):
    data = open(lib_path, "rb").read()
    assert b"gfx950" in data


def test_missing_library_fails_loudly(tmp_path):
    saved = _lib._lib
    _lib._lib = None
    try:
        with pytest.raises(_lib.RecalgoError):
            _lib.load(str(tmp_path / "nope.so"))
    finally:
        _lib._lib = saved


def imported_modules(path):
    """[(module, line)] of every absolute import of a source file: static scan"""
    import ast
    out = []
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.Import):
            out += [(a.name, node.lineno) for a in node.names]
        elif isinstance(node, ast.ImportFrom) and node.level == 0 and node.module:
            out.append((node.module, node.lineno))
    return out


def test_product_path_never_imports_the_oracle():
    """oracle/ is test infrastructure: only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg
    (a child process running `-m oracle.cpu_baseline`) may touch it.  Static scan of the product sources."""
    import glob
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    offenders = []
    for path in glob.glob(os.path.join(root, "recalgorithm_amd", "**", "*.py"), recursive=True) + [os.path.join(root, "bench.py")]:
        offenders += [f"{os.path.relpath(path, root)}:{line}" for m, line in imported_modules(path)
                      if m == "oracle" or m.startswith("oracle.")]
    assert not offenders, offenders
    # bench.py reaches the oracle only through the cpu_baseline child process
    src = open(os.path.join(root, "bench.py")).read()
    assert '"-m", "oracle.cpu_baseline"' in src
    # and the script that records what an ABI version covers takes it from the product, not from the test suite
    record = imported_modules(os.path.join(root, "scripts", "abi_record.py"))
    assert any(m == "recalgorithm_amd" for m, _ in record)
    assert not [m for m, _ in record if m == "tests" or m.startswith("tests.")]

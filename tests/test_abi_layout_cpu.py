"""include/aligner_hip.h against its two hand-written mirrors, without a GPU: the record layouts the C compiler gives the header
(printed by tests/abi_families.c) against the ctypes classes of aligner_amd/_ffi.py and the #[repr(C)] structs of
rust/aligner-core-hip/src/lib.rs, the header's prototypes against argtypes / restype and the Rust extern declarations, and the
condition that every declared function is called from one of the two C harnesses."""
import ctypes as C
import os
import re
import subprocess

import pytest

from aligner_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aligner_hip.h")
RUST = os.path.join(ROOT, "rust", "aligner-core-hip", "src", "lib.rs")
CLASSES = {"aln_params": _ffi.Params, "aln_pair_result": _ffi.PairResult, "aln_scan_geometry": _ffi.ScanGeometry,
           "aln_shuffle_spec": _ffi.ShuffleSpec, "aln_seqset_block": _ffi.SeqsetBlock, "aln_signif_record": _ffi.SignifRecord,
           "aln_hit_report": _ffi.HitReport, "aln_hit_filter": _ffi.HitFilter}
RENAMED = {("aln_params", "del_"): "del"}              # `del` is a Python keyword: the one rename a mirror may make


def strip_c_comments(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


@pytest.fixture(scope="module")
def printout():
    from aligner_amd import build as native_build
    native_build.build()
    exe = native_build.build_families_harness()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


@pytest.fixture(scope="module")
def header_layouts(printout):
    """{type: (sizeof, [(field, offset, size)])} as the C compiler lays the header out"""
    out = {}
    for line in printout.splitlines():
        w = line.split()
        if w and w[0] == "layout":
            assert (len(w) - 3) % 3 == 0, line
            out[w[1]] = (int(w[2]), [(w[i], int(w[i + 1]), int(w[i + 2])) for i in range(3, len(w), 3)])
    return out


def header_fields(name):
    """field names of a record in declaration order, read from the header's text"""
    text = strip_c_comments(open(HEADER).read())
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), text, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"^.*?(\w+)$", r"\1", part.strip()) for part in decl.split(",")]
    return names


def ctypes_layout(name, cls):
    fields = [(RENAMED.get((name, f), f), getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_]
    return C.sizeof(cls), fields


def test_versions_agree_and_every_record_is_printed(printout, header_layouts):
    assert "abi_version_header 2" in printout and "abi_version_library 2" in printout
    assert sorted(header_layouts) == sorted(CLASSES)
    for name, (size, fields) in header_layouts.items():
        assert [f for f, _, _ in fields] == header_fields(name), name          # the program lists every field, in the header's order
        assert fields[0][1] == 0 and all(a[1] + a[2] <= b[1] for a, b in zip(fields, fields[1:])) and fields[-1][1] + fields[-1][2] <= size


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_layout_equals_ctypes_mirror(header_layouts, name):
    assert ctypes_layout(name, CLASSES[name]) == header_layouts[name]


# ---------------------------------------------------------------- the Rust mirror, read as text
RUST_WIDTH = {"u8": 1, "i8": 1, "u32": 4, "i32": 4, "u64": 8, "i64": 8, "f64": 8, "usize": 8, "isize": 8}


def snake(camel):
    return re.sub(r"(?<!^)([A-Z])", r"_\1", camel).lower()


def rust_structs():
    """{c name: (size, [(field, offset, size)])} of the #[repr(C)] structs with named scalar / pointer fields, offsets by natural
    alignment (what repr(C) means on this ABI)"""
    text = re.sub(r"//[^\n]*", "", open(RUST).read())
    out = {}
    for m in re.finditer(r"#\[repr\(C\)\]\s*(?:#\[[^\]]*\]\s*)*pub struct (\w+)\s*\{(.*?)\}", text, flags=re.S):
        fields, off, align, opaque = [], 0, 1, False
        for decl in m.group(2).split(","):
            decl = decl.strip()
            if not decl:
                continue
            fm = re.match(r"(?:pub\s+)?(\w+)\s*:\s*(.+)$", decl, flags=re.S)
            assert fm, decl
            ty = fm.group(2).strip()
            if ty.startswith("["):                   # an opaque handle's zero-sized array
                opaque = True
                break
            w = 8 if ty.startswith("*") else RUST_WIDTH[ty]
            off = (off + w - 1) // w * w
            fields.append((fm.group(1), off, w))
            off += w
            align = max(align, w)
        if not opaque:
            out[snake(m.group(1))] = ((off + align - 1) // align * align, fields)
    return out


def test_layout_equals_rust_mirror(header_layouts):
    mirrors = rust_structs()
    assert {"aln_params", "aln_pair_result"} <= set(mirrors)                     # the parser found the file's structs
    compared = 0
    for name, layout in mirrors.items():
        if name in header_layouts:                                              # a struct lib.rs lacks is not a failure
            assert layout == header_layouts[name], name
            compared += 1
    assert compared >= 2


# ---------------------------------------------------------------- prototypes
C_KIND = {"int": "i32", "int32_t": "i32", "uint32_t": "u32", "uint64_t": "u64", "size_t": "u64", "double": "f64", "void": "void"}


def c_kind(decl, is_param):
    decl = decl.strip()
    if "*" in decl:
        return "pointer"
    words = [w for w in decl.split() if w != "const"]
    if is_param and len(words) > 1:
        words = words[:-1]                                                      # the parameter's name
    assert len(words) == 1, decl
    return C_KIND[words[0]]


def header_prototypes():
    """{function: (return kind, [parameter kinds])}"""
    text = strip_c_comments(open(HEADER).read())
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    text = re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", "", text, flags=re.S)
    text = re.sub(r"enum\s+\w+\s*\{.*?\}\s*;", "", text, flags=re.S)
    text = re.sub(r"typedef\s+struct\s+\w+\s+\w+\s*;", "", text)
    text = text.replace('extern "C" {', "")
    out = {}
    for m in re.finditer(r"([\w\s\*]+?)\b(aln_\w+)\s*\(([^)]*)\)\s*;", text):
        params = m.group(3).strip()
        kinds = [] if params in ("", "void") else [c_kind(p, True) for p in params.split(",")]
        out[m.group(2)] = (c_kind(m.group(1), False), kinds)
    return out


def ctypes_kind(t):
    if t is None:
        return "void"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return "pointer"
    return {"i": "i32", "I": "u32", "L": "u64", "Q": "u64", "l": "i64", "q": "i64", "d": "f64"}[t._type_]


def test_header_declares_what_the_mirror_exports():
    protos = header_prototypes()
    assert sorted(protos) == sorted(_ffi.EXPORTS) and len(protos) == 61


def test_prototypes_equal_ctypes_mirror():
    from aligner_amd import build as native_build
    native_build.build()
    lib = _ffi.load()
    for name, (ret, params) in sorted(header_prototypes().items()):
        fn = getattr(lib, name)
        assert fn.argtypes is not None, "%s: no argtypes set" % name
        assert (ctypes_kind(fn.restype), [ctypes_kind(t) for t in fn.argtypes]) == (ret, params), name


RUST_KIND = {"c_int": "i32", "i32": "i32", "u32": "u32", "c_uint": "u32", "u64": "u64", "usize": "u64", "f64": "f64", "i64": "i64"}


def rust_prototypes():
    text = re.sub(r"//[^\n]*", "", open(RUST).read())
    out = {}
    for m in re.finditer(r"\bfn\s+(aln_\w+)\s*\(([^)]*)\)\s*(?:->\s*([^;{]+?))?\s*;", text, flags=re.S):
        def kind(ty):
            ty = ty.strip()
            return "pointer" if ty.startswith("*") else RUST_KIND[ty]
        params = [kind(p.split(":", 1)[1]) for p in m.group(2).split(",") if p.strip()]
        out[m.group(1)] = (kind(m.group(3)) if m.group(3) else "void", params)
    return out


def test_prototypes_equal_rust_mirror():
    protos, rust = header_prototypes(), rust_prototypes()
    assert len(rust) >= 20 and "aln_align_batch" in rust                        # the parser found the file's declarations
    for name, sig in sorted(rust.items()):
        if name in protos:                                                      # a function lib.rs lacks is not a failure
            assert sig == protos[name], name
    assert set(rust) <= set(protos), sorted(set(rust) - set(protos))            # and it declares nothing the header does not


# ---------------------------------------------------------------- coverage
def test_every_declared_function_is_called_from_c():
    """Every function of the header is called by tests/abi_families.c or tests/abi_harness.c, so a new family cannot arrive without
    its C caller."""
    src = "".join(strip_c_comments(open(os.path.join(ROOT, "tests", f)).read()) for f in ("abi_families.c", "abi_harness.c"))
    src = re.sub(r'"(?:[^"\\\n]|\\.)*"', '""', src)                            # (a name inside a string literal is not a call)
    missing = [name for name in sorted(header_prototypes()) if not re.search(r"\b%s\s*\(" % name, src)]
    assert not missing, missing

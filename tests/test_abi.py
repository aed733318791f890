"""The C-ABI library loads and exports every symbol include/lemsm.h declares, and the two hand-kept copies of its signatures
-- the ctypes table of halo2_liam_eagen_msm_amd/_lib.py and the Rust declarations of INTEGRATION.md -- have the header's
arity and type classes (tests/abi_sig.py) (no GPU needed; no compute entry is called here)."""
import ctypes
import os
import re

from halo2_liam_eagen_msm_amd import _lib

import abi_sig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    text = open(os.path.join(ROOT, "include", "lemsm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lemsm_[a-z0-9_]+)\s*\(", text)))


def test_header_matches_binding_table():
    assert header_symbols() == sorted(_lib.SYMBOLS)


def _header_text():
    return open(os.path.join(ROOT, "include", "lemsm.h")).read()


def test_signature_parser_reports_doctored_prototypes():
    """the parser alone, no library: a one-line prototype reads as written, and each doctored copy of it -- size_t -> uint32_t, a
    dropped argument, size_t* -> uint32_t*, uint8_t base -> int base -- is reported against the unchanged one (without this the
    two signature tests below could pass by parsing nothing)"""
    proto = ("typedef struct lemsm_ctx lemsm_ctx;\n"
             "int lemsm_demo(lemsm_ctx* ctx, const uint8_t* scalars /* n x 32 */, size_t n, uint8_t base, const uint64_t x[4],\n"
             "               double out[3], const void* const* cols, size_t* bad_index);   // trailing\n")
    want = abi_sig.parse_header(proto)
    assert want == {"lemsm_demo": ("i4", ["*opaque", "*u1", "u8", "u1", "*u8", "*f8", "**", "*u8"])}
    assert abi_sig.mismatches(want["lemsm_demo"], want["lemsm_demo"]) == []
    doctored = {"size_t n": ("uint32_t n", "argument 2 is u4"), "size_t n, ": ("", "7 arguments, the header has 8"),
                "size_t* bad_index": ("uint32_t* bad_index", "argument 7 is *u4"), "uint8_t base": ("int base", "argument 3 is i4")}
    for old, (new, said) in doctored.items():
        assert proto.count(old) == 1
        got = abi_sig.parse_header(proto.replace(old, new))["lemsm_demo"]
        found = abi_sig.mismatches(want["lemsm_demo"], got)
        assert len(found) == 1 and found[0].startswith(said), (old, found)
        assert abi_sig.mismatches(got, want["lemsm_demo"]), old           # (and the other way round)
    # the same four against a ctypes and a Rust rendering of the unchanged prototype
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    bound = ["*any", "*any", "u8", "u1", "*any", "*f8", "**", "*u8"]
    assert [abi_sig.ctypes_class(t) for t in (vp, vp, sz, ctypes.c_uint8, vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(vp),
                                              ctypes.POINTER(sz))] == bound and abi_sig.ctypes_class(ctypes.c_int) == "i4"
    assert abi_sig.mismatches(want["lemsm_demo"], ("i4", bound)) == []
    rust = ("```rust\nextern \"C\" {\n    // fn lemsm_gone(a: i32);\n    pub fn lemsm_demo(ctx: *mut LemsmCtx, scalars: *const u8, n: usize, base: u8,\n"
            "        x: *const u64, out: *mut f64, cols: *const *const std::ffi::c_void, bad_index: *mut usize) -> c_int;\n}\n```\n")
    assert abi_sig.parse_rust(rust, proto) == want
    for old in doctored:
        got = abi_sig.parse_header(proto.replace(old, doctored[old][0]))["lemsm_demo"]
        assert abi_sig.mismatches(got, ("i4", bound)) and abi_sig.mismatches(got, abi_sig.parse_rust(rust, proto)["lemsm_demo"]), old
    assert abi_sig.mismatches(("i4", ["u8"]), ("i4", ["*any"])) and abi_sig.mismatches(("*i1", []), ("i4", []))


def test_binding_signatures_match_the_header():
    """restype and argtypes of every bound function have the header's arity and classes: c_void_p may stand for any pointer, a
    typed POINTER(T) must match the pointee's width and kind"""
    want = abi_sig.parse_header(_header_text())
    assert sorted(want) == sorted(_lib.SYMBOLS) and len(want) == 156
    _lib.build()
    lib = _lib.load()
    wrong = {}
    for name in _lib.SYMBOLS:
        found = abi_sig.mismatches(want[name], abi_sig.ctypes_signature(getattr(lib, name)))
        if found:
            wrong[name] = found
    assert not wrong, wrong


def test_rust_block_matches_the_header():
    """every `fn lemsm_*` of INTEGRATION.md's fenced rust blocks has the header's arity and classes (the document declares a part
    of the ABI: completeness is not asked)"""
    want = abi_sig.parse_header(_header_text())
    rust = abi_sig.parse_rust(open(os.path.join(ROOT, "INTEGRATION.md")).read(), _header_text())
    assert len(rust) >= 73 and set(rust) <= set(want), sorted(set(rust) - set(want))
    wrong = {name: found for name, found in ((n, abi_sig.mismatches(want[n], rust[n])) for n in rust) if found}
    assert not wrong, wrong


def test_library_builds_loads_and_exports_all():
    _lib.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in header_symbols():
        assert hasattr(lib, name), name


def test_no_oracle_in_product():
    """the product package must not import, link or execute anything under oracle/"""
    pkg = os.path.join(ROOT, "halo2_liam_eagen_msm_amd")
    for dirpath, _, files in os.walk(pkg):
        if "_build" in dirpath:
            continue
        for f in files:
            if f.endswith((".py", ".hip", ".cuh", ".h", ".hpp", "Makefile")):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r'#include\s+["<][^">]*oracle', text), f
                assert "oracle/_build" not in text and "oracle/c" not in text, f
                if f.endswith(".py"):
                    assert not re.search(r"^\s*(import oracle|from oracle)", text, re.M), f
                assert "liblemsm_oracle" not in text, f


def test_header_is_plain_c(tmp_path):
    """the boundary is a C ABI: include/lemsm.h compiles as C99 (no torch / C++ types in the signatures)
    and a C program links against the library and calls an entry that needs no GPU"""
    import subprocess
    src = tmp_path / "use.c"
    src.write_text(
        '#include "lemsm.h"\n#include <stdio.h>\n'
        "int main(void) {\n"
        "  uint32_t d = 0; uint64_t out[12]; uint64_t two[24] = {0};\n"
        "  if (lemsm_num_digits(LEMSM_GRUMPKIN, 5, &d) != LEMSM_OK) return 1;\n"
        "  if (lemsm_jacobian_sum(LEMSM_BN254_G1, two, 2, out) != LEMSM_OK) return 2;   /* identity + identity */\n"
        "  for (int i = 0; i < 12; i++) if (out[i]) return 3;\n"
        '  printf("%u\\n", d); return 0;\n}\n')
    exe = tmp_path / "use"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L", libdir, "-llemsm", "-Wl,-rpath," + libdir])
    out = subprocess.check_output([str(exe)]).decode().strip()
    from oracle import pyref
    assert int(out) == pyref.num_digits(pyref.GRUMPKIN.order, 5)

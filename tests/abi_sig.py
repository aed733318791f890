"""Signatures of the C ABI reduced to classes, from its three hand-kept copies (test infrastructure; tests/test_abi.py):
    parse_header(text)     every prototype of include/lemsm.h
    ctypes_signature(fn)   restype / argtypes of a bound function of halo2_liam_eagen_msm_amd/_lib.py
    parse_rust(text, ...)  every `fn lemsm_*` of the fenced rust blocks of INTEGRATION.md
each as (return class, [argument classes]).  A class is one of
    "void"                                    (a return only)
    "i1" "u1" "i4" "u4" "i8" "u8" "f8"        signed / unsigned integer of 1, 4, 8 bytes; double  (LP64: size_t = u8, long = i8)
    "*" + one of those                        a pointer to one (an array parameter is a pointer; const is ignored)
    "**"                                      a pointer to a pointer
    "*opaque"                                 void* or a pointer to a type declared without a body (lemsm_ctx, ...)
    "*struct"                                 a pointer to a struct the header lays out (lemsm_gate_program, ...)
    "*any"                                    ctypes' c_void_p only: it stands for any pointer
mismatches(want, got) lists where a copy leaves the header: arity first, then class by class."""
import ctypes
import re

C_SCALARS = {"void": "void", "char": "i1", "int": "i4", "long": "i8", "double": "f8", "size_t": "u8", "uint8_t": "u1", "int32_t": "i4",
             "uint32_t": "u4", "uint64_t": "u8", "int64_t": "i8"}
RUST_SCALARS = {"usize": "u8", "c_int": "i4", "i32": "i4", "u8": "u1", "u32": "u4", "u64": "u8", "f64": "f8", "c_long": "i8", "c_char": "i1",
                "c_void": "opaque"}


def strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def header_types(text):
    """{typedef name: "opaque" | "struct"} of a comment-free header"""
    types = {name: "opaque" for name in re.findall(r"typedef\s+struct\s+\w+\s+(\w+)\s*;", text)}
    types.update({name: "struct" for name in re.findall(r"typedef\s+struct\s*\w*\s*\{[^}]*\}\s*(\w+)\s*;", text)})
    return types


def c_class(decl, types):
    """the class of one C parameter or return type, with or without the parameter's name"""
    toks = [t for t in re.findall(r"[A-Za-z_]\w*|\*|\[[^\]]*\]", decl) if t != "const"]
    if not toks or toks[0] == "*" or toks[0].startswith("["):
        raise ValueError("no type in %r" % decl)
    base = toks[0]
    if base not in C_SCALARS and base not in types:
        raise ValueError("unknown type %r in %r" % (base, decl))
    rest = toks[1:]
    depth = 0
    while rest and rest[0] == "*":
        depth, rest = depth + 1, rest[1:]
    if rest and re.match(r"[A-Za-z_]", rest[0]):                   # the parameter's name
        rest = rest[1:]
    if rest and rest[0].startswith("["):
        depth, rest = depth + 1, rest[1:]
    if rest:
        raise ValueError("cannot read %r" % decl)
    kind = "opaque" if base == "void" else C_SCALARS.get(base) or types[base]
    if depth == 0:
        if kind in ("opaque", "struct") and base != "void":
            raise ValueError("%r passed by value in %r" % (base, decl))
        return "void" if base == "void" else kind
    return "**" if depth >= 2 else "*" + kind


def parse_header(text):
    """{name: (return class, [argument classes])} of every `lemsm_*(...)` prototype"""
    text = re.sub(r"^\s*#.*$", " ", strip_comments(text), flags=re.M)
    types = header_types(text)
    text = re.sub(r"typedef\s+struct\s*\w*\s*\{[^}]*\}\s*\w+\s*;", " ", text)
    out = {}
    for ret, name, args in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(lemsm_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        if name in out:
            raise ValueError("%s is declared twice" % name)
        args = [a.strip() for a in args.split(",")]
        out[name] = (c_class(ret, types), [] if args == ["void"] else [c_class(a, types) for a in args])
    return out


def ctypes_class(t):
    if t is None:
        return "void"
    if t is ctypes.c_void_p:
        return "*any"
    if t is ctypes.c_char_p:
        return "*i1"
    if isinstance(t, type) and issubclass(t, ctypes._Pointer):
        to = t._type_
        if to is ctypes.c_void_p or to is ctypes.c_char_p or (isinstance(to, type) and issubclass(to, ctypes._Pointer)):
            return "**"
        return "*struct" if issubclass(to, ctypes.Structure) else "*" + ctypes_class(to)
    if isinstance(t, type) and issubclass(t, ctypes._SimpleCData):
        code, size = t._type_, ctypes.sizeof(t)
        if code == "d":
            return "f8"
        if code in "bhilq":
            return "i%d" % size
        if code in "BHILQ":
            return "u%d" % size
    raise ValueError("no class for %r" % (t,))


def ctypes_signature(fn):
    if fn.argtypes is None:
        raise ValueError("no argtypes bound")
    return ctypes_class(fn.restype), [ctypes_class(a) for a in fn.argtypes]


def rust_class(decl, types):
    toks = decl.replace("*", " * ").split()
    depth = 0
    while len(toks) >= 2 and toks[0] == "*" and toks[1] in ("const", "mut"):
        depth, toks = depth + 1, toks[2:]
    if len(toks) != 1:
        raise ValueError("cannot read %r" % decl)
    base = toks[0].split("::")[-1]
    if base in RUST_SCALARS:
        kind = RUST_SCALARS[base]
    else:                                                          # LemsmGateProgram -> lemsm_gate_program
        kind = types.get(re.sub(r"(?<!^)([A-Z])", r"_\1", base).lower())
        if kind is None:
            raise ValueError("unknown type %r in %r" % (base, decl))
    if depth == 0:
        if kind in ("opaque", "struct"):
            raise ValueError("%r passed by value in %r" % (base, decl))
        return kind
    return "**" if depth >= 2 else "*" + kind


def parse_rust(markdown, header_text):
    """{name: (return class, [argument classes])} of every `fn lemsm_*` in the document's fenced rust blocks"""
    types = header_types(strip_comments(header_text))
    out = {}
    for block in re.findall(r"^```rust\n(.*?)^```", markdown, flags=re.S | re.M):
        block = re.sub(r"//[^\n]*", " ", block)
        for name, args, ret in re.findall(r"\bfn\s+(lemsm_[a-z0-9_]+)\s*\(([^()]*)\)\s*(?:->\s*([^;{]+?))?\s*[;{]", block):
            args = [a.split(":", 1)[1].strip() for a in args.split(",") if a.strip()]
            sig = ("void" if not ret else rust_class(ret, types), [rust_class(a, types) for a in args])
            if out.setdefault(name, sig) != sig:
                raise ValueError("%s is declared twice, differently" % name)
    return out


def mismatches(want, got):
    """where signature `got` leaves the header's `want`; "*any" in `got` stands for any pointer"""
    def same(w, g):
        return w == g or (g == "*any" and w.startswith("*"))
    if len(want[1]) != len(got[1]):
        return ["%d arguments, the header has %d" % (len(got[1]), len(want[1]))]
    bad = [] if same(want[0], got[0]) else ["returns %s, the header %s" % (got[0], want[0])]
    return bad + ["argument %d is %s, the header's %s" % (k, g, w) for k, (w, g) in enumerate(zip(want[1], got[1])) if not same(w, g)]

"""Reader of the project's C headers: the ctypes signatures and the constants of a binding come from the header itself.

Standard library only -- no torch, no unet_amd._lib, no shared object -- so unet_amd/tiffio.py can type libunet_tiff.so on a box without
the HIP runtime.  It reads the closed vocabulary include/unet_hip.h and include/unet_tiff.h are written in and nothing else, and it is
strict: a prototype, a type or a constant it cannot read raises AbiError naming it.  Nothing is skipped, so no function is ever left
with ctypes' default `int` signature.

Type mapping (signatures): int, unsigned, long long, unsigned long long, size_t, float, double by value; void as a return type;
`const char*` as a return type is c_char_p; a pointer to a struct of the header is POINTER(<its registered mirror class>); every other
pointer is c_void_p.  Known narrowing: a header cannot tell a host pointer (`const float* lr`, `int* th`) from a device pointer, so
host-side pointers are c_void_p too.  Callers pass a ctypes array, byref(), cast() or data_as() pointer there, all of which c_void_p
accepts; the one difference from a POINTER(c_float) spelling is that such a parameter would also accept a bare integer.

Struct bodies are not parsed: the mirror classes stay hand-written, and tests/test_abi_cpu.py has the C compiler compare their layout
with the header's.
"""
from __future__ import annotations

import ctypes as C
import re
from collections import Counter
from pathlib import Path
from typing import NamedTuple

_SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong, "size_t": C.c_size_t,
            "float": C.c_float, "double": C.c_double}
_TYPE_WORDS = {"const", "void", "char", "int", "unsigned", "signed", "short", "long", "float", "double", "size_t"}


class AbiError(ValueError):
    pass


class Decl(NamedTuple):
    name: str
    ret: str            # normalised C types: one space between words, every `*` attached ("const float*", "unsigned long long")
    params: tuple


def _text(path) -> str:
    """the header without its comments"""
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", " ", Path(path).read_text(), flags=re.S))


def _ctype(text: str, name: str, is_param: bool) -> str:
    text, _, dims = text.partition("[")                    # `T name[N]` is a pointer
    tok = text.replace("*", " * ").split()
    if is_param and len(tok) > 1 and tok[-1] != "*" and tok[-1] not in _TYPE_WORDS:
        tok.pop()                                          # the parameter's name
    words = [t for t in tok if t != "*"]
    if not words or not all(w.replace("_", "a").isalnum() for w in words):
        raise AbiError(f"{name}: cannot read `{' '.join(text.split())}`")
    return " ".join(words) + "*" * (len(tok) - len(words) + bool(dims))


def declarations(path) -> list:
    """Decl(name, ret, params) of every file-scope prototype `ret unet_name(params);`, in the header's order"""
    txt = _text(path)
    body = re.sub(r"^[ \t]*#.*$", "", txt, flags=re.M)
    body = re.sub(r'extern\s+"C"\s*\{', "", body)
    body = re.sub(r"\{[^{}]*\}", " ", body).replace("}", ";")          # struct / enum bodies; the brace that closes extern "C"
    out = []
    for stmt in map(str.strip, body.split(";")):
        if not stmt or stmt.startswith(("typedef", "enum")):
            continue
        m = re.fullmatch(r"(.+?)\b(unet_[a-z0-9_]+)\s*\((.*)\)", stmt, flags=re.S)
        if not m:
            raise AbiError(f"cannot read the declaration `{' '.join(stmt.split())}`")
        ret, name, params = m.groups()
        if "(" in params:
            raise AbiError(f"{name}: function-pointer parameter in `{' '.join(params.split())}`")
        parts = [] if params.strip() in ("", "void") else params.split(",")
        out.append(Decl(name, _ctype(ret, name, False), tuple(_ctype(p, name, True) for p in parts)))
    stray = Counter(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", txt)) - Counter(d.name for d in out)
    if stray:
        raise AbiError(f"`unet_...(` outside every prototype this reader parsed: {sorted(stray)}")
    return out


def constants(path) -> dict:
    """{name: value} of every `#define UNET_X <integer>` and every enumerator of the anonymous `enum { UNET_A = 1, ... };` blocks"""
    txt, out = _text(path), {}

    def value(name, s):
        m = re.fullmatch(r"\(?\s*(-?)\s*(0[xX][0-9a-fA-F]+|\d+)\s*\)?", s.strip())
        if not m:
            raise AbiError(f"{name}: `{s.strip()}` is not an integer")
        return int(m.group(1) + m.group(2), 0)

    for name, s in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(UNET_\w+)[ \t]+(\S.*)$", txt, flags=re.M):
        out[name] = value(name, s)
    for block in re.findall(r"\benum\s*\{([^{}]*)\}\s*;", txt):
        nxt = 0
        for item in filter(None, map(str.strip, block.split(","))):
            name, eq, s = map(str.strip, item.partition("="))
            out[name] = value(name, s) if eq else nxt
            nxt = out[name] + 1
    return out


def struct_names(path) -> list:
    """the name of every `typedef struct ... { ... } unet_x;`"""
    return re.findall(r"\btypedef\s+struct\b[^{};]*\{[^{}]*\}\s*(\w+)\s*;", _text(path))


def signatures(path, structs: dict, only=None) -> dict:
    """{name: (restype, [argtypes])} of the header's prototypes: all of them, or those named in `only`.  structs maps the header's struct
    typedefs to their mirror classes: every one of them for the whole header, those the prototypes of `only` point to otherwise."""
    known = struct_names(path)
    decls = [d for d in declarations(path) if only is None or d.name in only]
    absent = sorted(set(only or ()) - {d.name for d in decls})
    if absent:
        raise AbiError(f"{path} does not declare {absent}")

    def mirror(s, name):
        if s not in structs:
            raise AbiError(f"{name}: struct typedef `{s}` has no registered mirror class")
        return structs[s]

    def ctype(t, name, is_ret=False):
        if not t.endswith("*"):
            if is_ret and t == "void":
                return None
            if t not in _SCALARS:
                raise AbiError(f"{name}: type `{t}` is outside the vocabulary of this reader")
            return _SCALARS[t]
        if is_ret and t == "const char*":
            return C.c_char_p
        base = " ".join(w for w in t.rstrip("*").split() if w != "const")
        return C.POINTER(mirror(base, name)) if base in known and t.count("*") == 1 else C.c_void_p

    if only is None:
        for s in known:
            mirror(s, Path(path).name)
    return {d.name: (ctype(d.ret, d.name, True), [ctype(p, d.name) for p in d.params]) for d in decls}

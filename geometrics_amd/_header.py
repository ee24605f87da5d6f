"""The C ABI as include/geom_hip.h declares it, read once at import: the one description of the boundary (no torch here).

    PROTOTYPES  name -> (restype, argtypes)              every `geom_*` function
    STRUCTS     name -> ctypes.Structure subclass        every `typedef struct name { ... } name;`, fields in header order
    CONSTANTS   X -> int                                 every `#define GEOM_X <integer>`, written 16, 16u or (-3)

Accepted declarations are those of the header's conventions block; anything else raises -- a type is never guessed."""
import ctypes
import os
import re

from .build import INCLUDE

PATH = os.path.join(INCLUDE, "geom_hip.h")
SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float, "int64_t": ctypes.c_int64,
           "size_t": ctypes.c_size_t}


def _ctype(base, pointer, where):
    """`base` = a declaration's type words without its `*`s and its name."""
    if pointer:
        return ctypes.c_void_p
    base = " ".join(w for w in base.split() if w != "const")
    if base not in SCALARS:
        raise RuntimeError("geom_hip.h: type %r in `%s` is none the binding knows (%s, or a pointer)"
                           % (base, " ".join(where.split()), ", ".join(SCALARS)))
    return SCALARS[base]


def _fields(body, where):
    """`const float *a, *b; int x;` -> [(a, void*), (b, void*), (x, int)]: the first declarator carries the base type."""
    out = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        base = None
        for piece in decl.split(","):
            prefix, name = re.fullmatch(r"(.*?)(\w+)\s*", piece, re.S).groups()
            base = prefix.replace("*", " ") if base is None else base
            out.append((name, _ctype(base, "*" in prefix, where + ": " + decl)))
    return out


def parse(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+GEOM_(\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M):
        m = re.fullmatch(r"\((-?\d+)\)|(\d+)u?", value)
        if not m:
            raise RuntimeError("geom_hip.h: #define GEOM_%s %s is not an integer the binding can read" % (name, value))
        constants[name] = int(m.group(1) or m.group(2))
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    structs = {}
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", text):
        structs[m.group(3)] = type(m.group(3), (ctypes.Structure,), {"_fields_": _fields(m.group(2), "struct " + m.group(1))})
    prototypes = {}
    for m in re.finditer(r"([\w\s*]+?)\b(geom_\w+)\s*\(([^(){};]*)\)\s*;", text):
        ret, name, params = m.groups()
        where = m.group(0)
        if " ".join(ret.split()) == "const char *":
            restype = ctypes.c_char_p
        else:
            restype = _ctype(ret, "*" in ret, where)
            if restype is ctypes.c_void_p:
                raise RuntimeError("geom_hip.h: `%s` returns a pointer other than const char *" % " ".join(where.split()))
        if params.strip() == "void":
            argtypes = []
        else:
            argtypes = [_ctype(re.sub(r"\w+\s*$", "", p).replace("*", " "), "*" in p, where) for p in params.split(",")]
        prototypes[name] = (restype, argtypes)
    mentioned = len(re.findall(r"\bgeom_\w+\s*\(", text))
    if mentioned != len(prototypes):
        raise RuntimeError("geom_hip.h: %d `geom_*(` occurrences but %d prototypes the binding could read (accepted: "
                           "`type geom_name(type name, ...);`, one name once)" % (mentioned, len(prototypes)))
    return prototypes, structs, constants


try:
    with open(PATH) as _f:
        _text = _f.read()
except OSError as e:
    raise RuntimeError("geometrics_amd: cannot read %s (%s) -- the ctypes binding is derived from it; there is no built-in "
                       "copy of the ABI" % (PATH, e))
PROTOTYPES, STRUCTS, CONSTANTS = parse(_text)

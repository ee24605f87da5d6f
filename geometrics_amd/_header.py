"""The C ABI as include/geom_hip.h declares it, read once at import: the one description of the boundary (no torch here).

    PROTOTYPES  name -> (restype, argtypes)              every `geom_*` function
    STRUCTS     name -> ctypes.Structure subclass        every `typedef struct name { ... } name;`, fields in header order
    CONSTANTS   X -> int                                 every `#define GEOM_X <integer>`, written 16, 16u or (-3)
    PARAMETERS  name -> [(parameter, pointee, depth)]    every function's parameters and every struct's fields, in order:
                                                         ("n", "scalar", 0), ("col", "int", 1), ("tensors", "float", 2),
                                                         ("cull", "geom_surface_cull", 1), ("stream", "void", 1)

PROTOTYPES and STRUCTS bind every pointer as an untyped one; PARAMETERS keeps what the header says it points to.
Accepted declarations are those of the header's conventions block; anything else raises -- a type is never guessed."""
import ctypes
import os
import re

from .build import INCLUDE

PATH = os.path.join(INCLUDE, "geom_hip.h")
SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float, "int64_t": ctypes.c_int64,
           "size_t": ctypes.c_size_t}
POINTEES = ("float", "int", "int64_t", "uint16_t", "uint64_t", "unsigned", "void")      # or a struct declared further up


def _ctype(base, depth, where, structs=()):
    """`base` = a declaration's type words without its `*`s and its name, `depth` = how many `*`s -> (ctype, pointee)."""
    base = " ".join(w for w in base.split() if w != "const")
    known = POINTEES + tuple(structs) if depth else tuple(SCALARS)
    if base not in known:
        raise RuntimeError("geom_hip.h: type %r in `%s` is none the binding knows (%s%s)"
                           % (base + " *" * depth, " ".join(where.split()), ", ".join(known), "" if depth else ", or a pointer"))
    return (ctypes.c_void_p, base) if depth else (SCALARS[base], "scalar")


def _fields(body, where, structs=()):
    """`const float *a, *b; int x;` -> ([(a, void*), (b, void*), (x, int)], [(a, float, 1), (b, float, 1), (x, scalar, 0)]):
    the first declarator carries the base type."""
    out, described = [], []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        base = None
        for piece in decl.split(","):
            prefix, name = re.fullmatch(r"(.*?)(\w+)\s*", piece, re.S).groups()
            base = prefix.replace("*", " ") if base is None else base
            ctype, pointee = _ctype(base, prefix.count("*"), where + ": " + decl, structs)
            out.append((name, ctype))
            described.append((name, pointee, prefix.count("*")))
    return out, described


def describe(text):
    """(prototypes, structs, constants, parameters) of a header's text."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+GEOM_(\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M):
        m = re.fullmatch(r"\((-?\d+)\)|(\d+)u?", value)
        if not m:
            raise RuntimeError("geom_hip.h: #define GEOM_%s %s is not an integer the binding can read" % (name, value))
        constants[name] = int(m.group(1) or m.group(2))
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    structs, parameters = {}, {}
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", text):
        fields, parameters[m.group(3)] = _fields(m.group(2), "struct " + m.group(1), structs)
        structs[m.group(3)] = type(m.group(3), (ctypes.Structure,), {"_fields_": fields})
    prototypes = {}
    for m in re.finditer(r"([\w\s*]+?)\b(geom_\w+)\s*\(([^(){};]*)\)\s*;", text):
        ret, name, params = m.groups()
        where = m.group(0)
        if " ".join(ret.split()) == "const char *":
            restype = ctypes.c_char_p
        elif "*" in ret:
            raise RuntimeError("geom_hip.h: `%s` returns a pointer other than const char *" % " ".join(where.split()))
        else:
            restype = _ctype(ret, 0, where)[0]
        argtypes, described = [], []
        for p in ([] if params.strip() == "void" else params.split(",")):
            ctype, pointee = _ctype(re.sub(r"\w+\s*$", "", p).replace("*", " "), p.count("*"), where, structs)
            argtypes.append(ctype)
            described.append((re.search(r"(\w+)\s*$", p).group(1), pointee, p.count("*")))
        prototypes[name], parameters[name] = (restype, argtypes), described
    mentioned = len(re.findall(r"\bgeom_\w+\s*\(", text))
    if mentioned != len(prototypes):
        raise RuntimeError("geom_hip.h: %d `geom_*(` occurrences but %d prototypes the binding could read (accepted: "
                           "`type geom_name(type name, ...);`, one name once)" % (mentioned, len(prototypes)))
    return prototypes, structs, constants, parameters


def parse(text):
    """(prototypes, structs, constants) of a header's text: the binding without what its pointers point to."""
    return describe(text)[:3]


try:
    with open(PATH) as _f:
        _text = _f.read()
except OSError as e:
    raise RuntimeError("geometrics_amd: cannot read %s (%s) -- the ctypes binding is derived from it; there is no built-in "
                       "copy of the ABI" % (PATH, e))
PROTOTYPES, STRUCTS, CONSTANTS, PARAMETERS = describe(_text)

"""CPU: the ctypes binding is what include/geom_hip.h says -- the reader's grammar on a synthetic header, the argument structs'
layout against the host C compiler, and the limits the python side uses against the header's #defines."""
import ctypes
import os
import re
import subprocess

import pytest

from geometrics_amd import _header, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "geom_hip.h")

_vp, _i, _u, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_float

SYNTHETIC = """
/* a comment with ( and ; and geom_not_a_function(int x); in it */
#ifndef GEOM_HIP_H
#define GEOM_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#define GEOM_ABI_VERSION 3
#define GEOM_FLAG_X 16u   /* geom_flag( ; */
#define GEOM_EBAD   (-3)  /* a comment that
                             runs on: geom_more(int); */
int geom_version(void);
const char *geom_strerror(int code);
typedef struct geom_args {
    int b, nv;
    const float *a, *b2; int x; float y, z;      /* [nv] or NULL; geom_inside(1) */
    const int64_t *faces; size_t bytes; unsigned flags; int64_t n;
} geom_args;
size_t geom_bytes(int b, int64_t n, size_t have);
int64_t geom_words(unsigned flags, float scale);
int geom_launch(int count, const float *const *tensors, const geom_args *args, uint16_t *mask,
                float *out, void *stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_reader_parses_every_accepted_form_exactly():
    prototypes, structs, constants = _header.parse(SYNTHETIC)
    assert constants == {"ABI_VERSION": 3, "FLAG_X": 16, "EBAD": -3}
    assert list(structs) == ["geom_args"] and issubclass(structs["geom_args"], ctypes.Structure)
    assert structs["geom_args"]._fields_ == [("b", _i), ("nv", _i), ("a", _vp), ("b2", _vp), ("x", _i), ("y", _f), ("z", _f),
                                             ("faces", _vp), ("bytes", ctypes.c_size_t), ("flags", _u), ("n", ctypes.c_int64)]
    assert prototypes == {
        "geom_version": (_i, []),
        "geom_strerror": (ctypes.c_char_p, [_i]),
        "geom_bytes": (ctypes.c_size_t, [_i, ctypes.c_int64, ctypes.c_size_t]),
        "geom_words": (ctypes.c_int64, [_u, _f]),
        "geom_launch": (_i, [_i, _vp, _vp, _vp, _vp, _vp]),
    }
    scalar = lambda *names: [(n, "scalar", 0) for n in names]
    described = _header.describe(SYNTHETIC)
    assert described[0] == prototypes and list(described[1]) == list(structs) and described[2] == constants
    assert described[3] == {
        "geom_version": [],
        "geom_strerror": scalar("code"),
        "geom_args": scalar("b", "nv") + [("a", "float", 1), ("b2", "float", 1)] + scalar("x", "y", "z")
        + [("faces", "int64_t", 1)] + scalar("bytes", "flags", "n"),
        "geom_bytes": scalar("b", "n", "have"),
        "geom_words": scalar("flags", "scale"),
        "geom_launch": scalar("count") + [("tensors", "float", 2), ("args", "geom_args", 1), ("mask", "uint16_t", 1),
                                          ("out", "float", 1), ("stream", "void", 1)],
    }


@pytest.mark.parametrize("declaration, complaint", [
    ("int geom_f(long n, void *stream);", "long"),                                   # a scalar the mapping does not hold
    ("int geom_f(double x);", "double"),
    ("int geom_f(geom_args args, void *stream);", "geom_args"),                      # a struct by value
    ("short geom_f(int n);", "short"),
    ("float *geom_f(int n);", "returns a pointer"),
    ("typedef struct geom_s { int a; double d; } geom_s;", "double"),
    ("int geom_f(const double *x);", "double *"),                                    # a pointee the mapping does not hold
    ("typedef struct geom_s { int a; const short *d; } geom_s;", "short *"),
    ("int geom_f(const geom_later *args, void *stream);", "geom_later *"),           # a struct nothing declares
    ("int geom_f(int (*callback)(int), void *stream);", "occurrences"),              # nothing the grammar can consume
    ("int geom_f(int n) { return n; }", "occurrences"),
    ("int geom_version(void);", "occurrences"),                                      # declared twice
    ("#define GEOM_LIMIT (1 << 4)", "GEOM_LIMIT"),
])
def test_reader_refuses_what_it_cannot_read(declaration, complaint):
    at = SYNTHETIC.index("size_t geom_bytes")
    with pytest.raises(RuntimeError, match=re.escape(complaint)):
        _header.parse(SYNTHETIC[:at] + declaration + "\n" + SYNTHETIC[at:])


def test_a_missing_header_fails_loudly(tmp_path):
    """The module reads the header at import: run its source against a directory without one."""
    source = open(_header.__file__).read().replace("from .build import INCLUDE", "INCLUDE = %r" % str(tmp_path))
    with pytest.raises(RuntimeError, match="cannot read .*geom_hip.h"):
        exec(compile(source, "_header_without_a_header", "exec"), {"__name__": "_header_without_a_header"})


def test_struct_layouts_are_the_c_compilers(tmp_path):
    """sizeof and every offsetof of every argument struct, as the host C compiler lays the real header out."""
    assert len(_header.STRUCTS) >= 5
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "geom_hip.h"', "int main(void) {"]
    for name, cls in _header.STRUCTS.items():
        lines.append('    printf("%s sizeof %%zu\\n", sizeof(%s));' % (name, name))
        for field, _ in cls._fields_:
            lines.append('    printf("%s %s %%zu\\n", offsetof(%s, %s));' % (name, field, name, field))
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, timeout=120)
    out = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True, timeout=60).stdout
    expected = {(a, b): int(c) for a, b, c in (line.split() for line in out.splitlines())}
    got = {}
    for name, cls in _header.STRUCTS.items():
        got[(name, "sizeof")] = ctypes.sizeof(cls)
        for field, _ in cls._fields_:
            got[(name, field)] = getattr(cls, field).offset
    assert got == expected
    assert len(expected) == sum(1 + len(cls._fields_) for cls in _header.STRUCTS.values())


def test_every_pointer_of_the_real_header_has_a_dtype_rule():
    """Each pointer parameter and field points to an argument struct or to a type the call boundary's dtype table knows."""
    assert set(_header.PARAMETERS) == set(_header.PROTOTYPES) | set(_header.STRUCTS)
    pointers = 0
    for name, described in _header.PARAMETERS.items():
        fields = _header.STRUCTS[name]._fields_ if name in _header.STRUCTS else None
        ctypes_of = [t for _, t in fields] if fields else _header.PROTOTYPES[name][1]
        assert len(described) == len(ctypes_of), name
        for (param, pointee, depth), ctype in zip(described, ctypes_of):
            assert (depth > 0) == (ctype is _vp) and (depth == 0) == (pointee == "scalar"), (name, param)
            if depth:
                pointers += 1
                assert depth in (1, 2) and (pointee in _lib.ADMITS or (pointee in _header.STRUCTS and depth == 1)), (name, param)
        if fields:
            assert [f for f, _ in fields] == [p for p, _, _ in described], name
    assert pointers > 500


def test_python_limits_are_the_headers():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    defined = dict(re.findall(r"^\s*#\s*define\s+GEOM_(\w+)[ \t]+\(?(-?\d+)u?\)?\s*$", text, flags=re.M))
    assert len(defined) >= 20 and {k: int(v) for k, v in defined.items()} == _header.CONSTANTS
    for name in ("ABI_VERSION", "EUNSUPPORTED", "FLAG_REF_TAIL_TRUNC", "FLAG_FIX_REGION6", "FLAG_TRI_BRUTE_FORCE", "FLAG_NN_FMA",
                 "FLAG_TRI_WS_READY", "ADAM_MAX_TENSORS", "ADAM_STATE_WORDS", "COLSUM_MAX_JOBS", "DENSE_MAX_LAYERS",
                 "DENSE_MAX_REDUCE_JOBS", "SUM_MAX_TENSORS"):
        assert getattr(_lib, name) == int(defined[name]), name
    for pyname, cname in (("DeformFwd", "geom_deform_fwd"), ("DeformBwd", "geom_deform_bwd"), ("DeformInfer", "geom_deform_infer"),
                          ("SurfaceCull", "geom_surface_cull"), ("SurfaceTail", "geom_surface_tail")):
        assert getattr(_lib, pyname) is _header.STRUCTS[cname]
    from geometrics_amd import deform
    assert deform.TAIL == int(defined["DEFORM_TAIL"]) and deform.WIDE_MAX_BATCH == int(defined["DEFORM_WIDE_MAX_B"])
    assert deform.LAYERS == 13 <= int(defined["DEFORM_CHAIN_MAX"])


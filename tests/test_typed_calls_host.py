"""CPU: what _lib.convert makes of the arguments of an entry point, without calling anything in the library."""
import ctypes

import pytest
import torch

from geometrics_amd import _header, _lib


def test_ints_none_and_ctypes_objects_pass_unchanged():
    wrote = ctypes.c_int(0)
    by_ref, array = ctypes.byref(wrote), (ctypes.c_int * 3)(1, 2, 3)
    given = [2, 162, None, 0x7f0000001000, array, by_ref, 1, ctypes.c_void_p(64)]
    out, device = _lib.convert("geom_laplacian_f32", given)
    assert device is None and len(out) == len(given) and all(a is b for a, b in zip(out, given))
    plan = _lib._plans["geom_laplacian_f32"]      # worked out once per entry point, then reused
    _lib.convert("geom_laplacian_f32", given)
    assert _lib._plans["geom_laplacian_f32"] is plan
    assert plan[0] == 8 and [p[:4] for p in plan[1]] == [(2, "rowptr", "int *", 1), (3, "col", "int *", 1), (4, "inv_deg", "float *", 1),
                                                         (5, "x", "float *", 1), (7, "out", "float *", 1)]


def test_a_cpu_tensor_is_refused_by_entry_point_and_parameter():
    col = torch.zeros(8, dtype=torch.int32)
    with pytest.raises(RuntimeError, match=r"geom_laplacian_f32: parameter `col` \(declared `int \*col`\) was given a torch.int32 "
                                           r"tensor on cpu -- it must live on a HIP device"):
        _lib.convert("geom_laplacian_f32", [2, 162, None, col, None, None, 0, None])
    with pytest.raises(RuntimeError, match=r"geom_sum_tensors_f32: parameter `tensors` \(declared `float \*\*tensors`\).*on cpu"):
        _lib.convert("geom_sum_tensors_f32", [2, [None, torch.zeros(4)], 4, None])
    with pytest.raises(RuntimeError, match="geom_sum_tensors_f32: parameter `tensors`.*takes a list of tensors"):
        _lib.convert("geom_sum_tensors_f32", [1, torch.zeros(4), 4, None])
    with pytest.raises(RuntimeError, match="geom_sum_f32: parameter `x`.*takes no list"):
        _lib.convert("geom_sum_f32", [4, [None], 1.0, None])
    with pytest.raises(RuntimeError, match=r"geom_surface_cull: parameter `gt_order` \(declared `int \*gt_order`\).*on cpu"):
        _lib.args(_lib.SurfaceCull, col, None, None, None)


def test_a_struct_goes_by_reference_and_only_where_it_is_declared():
    cull = _lib.args(_lib.SurfaceCull, None, 4096, None, None)
    assert cull.gt_index == 4096 and cull.gt_order is None
    names = [p for p, _, _ in _header.PARAMETERS["geom_surface_scan_f32"]][:-1]
    given = [None] * len(names)
    given[names.index("cull")] = cull
    out, _ = _lib.convert("geom_surface_scan_f32", given)
    by_ref = out[names.index("cull")]
    assert type(by_ref) is type(ctypes.byref(cull)) and by_ref._obj is cull
    given[names.index("cull")], given[names.index("tail")] = None, cull
    with pytest.raises(RuntimeError, match=r"geom_surface_scan_f32: parameter `tail` \(declared `geom_surface_tail \*tail`\) was "
                                           r"given a geom_surface_cull"):
        _lib.convert("geom_surface_scan_f32", given)
    # a host array of structs, as the chain launches take it
    layers = [_lib.args(_lib.DeformFwd, *([3] * 5 + [None] * 10 + [1, 0.1, 1e-5, 1, None, 0, 0.5] + [None] * 8 + [0])) for _ in range(2)]
    out, _ = _lib.convert("geom_deform_chain_fwd_f32", [2, layers, None])
    assert isinstance(out[1], _lib.DeformFwd * 2) and out[1][1].nv == 3 and abs(out[1][1].scale - 0.5) < 1e-7
    with pytest.raises(RuntimeError, match="geom_deform_chain_fwd_f32: parameter `layers`.*was given a geom_surface_cull"):
        _lib.convert("geom_deform_chain_fwd_f32", [1, [cull], None])


def test_a_wrong_argument_count_names_the_entry_point():
    with pytest.raises(RuntimeError, match=r"geom_sum_f32 takes 4 arguments and the stream \(3 given\)"):
        _lib.convert("geom_sum_f32", [4, None, 1.0])
    with pytest.raises(RuntimeError, match=r"geom_surface_cull takes 4 arguments \(5 given\)"):
        _lib.args(_lib.SurfaceCull, None, None, None, None, None)
    with pytest.raises(RuntimeError, match="geom_abi_version takes no stream"):
        _lib.convert("geom_abi_version", [])


def test_the_dtype_table_is_the_one_the_package_needs():
    assert _lib.ADMITS == {"float": (torch.float32,), "int": (torch.int32,), "int64_t": (torch.int64,), "uint16_t": (torch.int16,),
                           "uint64_t": (torch.int64,), "void": None}

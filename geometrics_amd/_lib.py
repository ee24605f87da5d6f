"""ctypes binding of libgeom_hip.so (the C ABI declared in include/geom_hip.h).

torch is used only for device memory and the current HIP stream; the signatures below are
plain pointers and sizes.  Loading fails loudly -- there is no fallback implementation.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libgeom_hip.so")

FLAG_REF_TAIL_TRUNC = 1
FLAG_FIX_REGION6 = 2
FLAG_TRI_BRUTE_FORCE = 4
FLAG_NN_FMA = 8
FLAG_TRI_WS_READY = 16
ABI_VERSION = 16
EUNSUPPORTED = -3
ADAM_MAX_TENSORS = 64
COLSUM_MAX_JOBS = 32
DENSE_MAX_LAYERS = 8
DENSE_MAX_REDUCE_JOBS = 32
ADAM_STATE_WORDS = 2112

# ---- package-wide reference-quirk mode (SURVEY quirk register Q1 / Q3) ------------------------------------------------
# The shipped CUDA kernels drop the tail of every 512-wide tile of targets / triangles (chamfer_distance.cu:31-33,
# tri_distance.cu:129,134); the default here is the full scan (= the reference's CPU nnsearch and its legacy kernels).
# With the mode on, every call that does not pass flags of its own -- ChamferDistance(), TriDistance(), chamfer_nn(),
# tri_distance(), batch_point_to_point / _surface, the compiled forward_cuda entry points -- reproduces the truncation
# exactly (GEOM_FLAG_REF_TAIL_TRUNC): what an unmodified driver needs to re-obtain the numbers of the reference's CUDA
# build, e.g. its validation F1 at 2466 points (GEOMetrics.py:227,349), where the last 2 targets are never seen.
_reference_quirks = os.environ.get("GEOM_REF_QUIRKS", "0") not in ("", "0")


def set_reference_quirks(on=True):
    """Switch the package-wide reference-quirk mode (initial value: environment variable GEOM_REF_QUIRKS)."""
    global _reference_quirks
    _reference_quirks = bool(on)
    from . import _shim
    if _shim._module is not None:          # the compiled entry points keep their own copy of the switch
        _shim._module.set_reference_quirks(_reference_quirks)
    return _reference_quirks


def reference_quirks():
    return _reference_quirks


def quirk_flags():
    """Flags of a call that passes none: GEOM_FLAG_REF_TAIL_TRUNC in reference-quirk mode, else 0."""
    return FLAG_REF_TAIL_TRUNC if _reference_quirks else 0


_vp = ctypes.c_void_p
_i = ctypes.c_int
_u = ctypes.c_uint
_f = ctypes.c_float

# name -> argtypes; every function returns int (0 ok / hipError_t / negative GEOM_E*)
_SIGNATURES = {
    "geom_chamfer_nn_f32": [_i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _u, _vp],
    "geom_chamfer_nn_culled_f32": [_i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u, _vp, _vp],
    "geom_tri_distance_f32": [_i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _u, _vp],
    "geom_tri_distance_indexed_f32": [_i, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _u, _vp],
    "geom_tri_distance_ws_f32": [_i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u, _vp, ctypes.c_size_t, _vp],
    "geom_tri_surface_fwd_f32": [_i, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u, _vp, ctypes.c_size_t, _vp],
    "geom_tri_distance_indexed_ws_f32": [_i, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _u, _vp, ctypes.c_size_t, _vp],
    "geom_face_areas_f32": [_i, _i, _vp, _i, _vp, _vp, _vp],
    "geom_draw_samples_f32": [_i, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp],
    "geom_draw_samples_rng_f32": [_i, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp],
    "geom_surface_loss_bwd_f32": [_i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _vp],
    "geom_surface_finalize_f32": [_i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _i,
                                  _i, _vp, _vp, _vp],
    "geom_surface_prepare_f32": [_i, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _u, _vp, ctypes.c_size_t, _vp, _vp, _vp],
    "geom_nn_cull_index_f32": [_i, _i, _vp, _vp, _vp, _vp],
    "geom_surface_scan_f32": [_i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                              _vp, _vp, _f, _f, _vp, _u, _vp, ctypes.c_size_t, _vp, _vp, _vp, _vp],
    "geom_surface_gather_f32": [_i, _i, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp],
    "geom_surface_finalize_w_f32": [_i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _i,
                                    _i, _vp, _vp, _vp, _vp],
    "geom_surface_gather_w_f32": [_i, _i, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp],
    "geom_vertex_head_fwd_f32": [ctypes.c_int64, _i, _vp, _vp, _f, _vp, _vp],
    "geom_vertex_head_bwd_f32": [ctypes.c_int64, _i, _vp, _f, _vp, _vp],
    "geom_sample_faces_fwd_f32": [_i, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp],
    "geom_sample_faces_bwd_f32": [_i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp],
    "geom_chamfer_grad_f32": [_i, _i, _vp, _i, _vp, _vp, _vp, _f, _vp, _i, _vp, _vp],
    "geom_p2tri_loss_fwd_f32": [_i, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "geom_p2tri_loss_bwd_f32": [_i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp],
    "geom_segment_max_fwd_f32": [_i, _vp, ctypes.c_int64, _i, _vp, _vp, _vp, _vp, ctypes.c_int64, _vp],
    "geom_segment_max_bwd_f32": [_i, _vp, ctypes.c_int64, _i, _vp, _vp, _vp, _vp],
    "geom_sum_f32": [ctypes.c_int64, _vp, _f, _vp, _vp],
    "geom_sample_chamfer_bwd_f32": [_i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _f, _vp, _vp],
    "geom_laplacian_f32": [_i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp],
    "geom_edge_sqlen_fwd_f32": [_i, _i, _vp, _i, _vp, _vp, _vp],
    "geom_edge_sqlen_bwd_f32": [_i, _i, _vp, _i, _vp, _vp, _f, _vp, _vp],
    "geom_vertex_bn_fwd_f32": [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _f, _f, _i, _vp, _i, _f, _vp, _vp, _vp, _vp],
    "geom_vertex_bn_bwd_f32": [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp],
    "geom_pool_features_fwd_ld_f32": [_i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, ctypes.c_int64, _vp],
    "geom_pool_features_fwd_fronts_f32": [_i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, ctypes.c_int64, _i, _vp, _vp, _vp, _vp, _vp],
    "geom_pool_features_bwd_ld_f32": [_i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, ctypes.c_int64, _vp, _vp, _vp, ctypes.c_size_t, _vp],
    "geom_colsum_batch_f32": [_i, _vp, _vp, _vp, _vp, _vp],
    "geom_adam_step_f32": [_i, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _vp, _i, _vp],
    "geom_adam_table_step_f32": [_i, _vp, ctypes.c_int64, _vp, _f, _f, _f, _f, _vp, _i, _vp],
    "geom_dense_fwd_f32": [_i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp],
    "geom_dense_bwd_input_f32": [_i, _i, _i, _vp, _vp, _vp, _vp],
    "geom_dense_bwd_weight_f32": [_i, _i, _i, _vp, _vp, _vp, _i, _vp],
    "geom_dense_bwd_f32": [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp],
    "geom_dense_reduce2_f32": [_i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp],
    "geom_dense_reduce_adam_f32": [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f,
                                   _vp, _vp],
    "geom_dense_reduce_f32": [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "geom_zn_gcn_aggregate_fwd_f32": [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp],
    "geom_zn_gcn_aggregate_ell_fwd_f32": [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp],
    "geom_zn_gcn_aggregate_ell_bwd_f32": [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp],
    "geom_zn_gcn_aggregate_ell_head_fwd_f32": [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _f, _vp, _vp],
    "geom_zn_gcn_aggregate_ell_head_bwd_f32": [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _i, _vp, _vp, _vp, _vp],
    "geom_zn_gcn_aggregate_bwd_f32": [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp],
    "geom_gemm_f32": [_i, _i, _i, _vp, ctypes.c_int64, _i, _vp, ctypes.c_int64, _i, _vp, ctypes.c_int64, _vp, ctypes.c_int64, _vp],
    "geom_zn_layer_fwd_f32": [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp],
    "geom_zn_layer_bwd_f32": [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _f, _vp, _i, _vp, _vp, _vp, _vp],
    "geom_camera_info_f32": [_i, _vp, _vp, _vp, _vp],
    "geom_sum_tensors_f32": [_i, _vp, ctypes.c_int64, _vp, _vp],
    "geom_sum_tensors_rows_f32": [_i, _vp, _vp, ctypes.c_int64, _i, _vp, _vp],
    "geom_split_bf16_planes_f32": [_i, _i, _vp, _vp, _vp],
    "geom_gemm_split_bf16_f32": [_i, _i, _i, _vp, _vp, _vp, _i, _vp],
    "geom_stage_regularisers_fwd_f32": [_i, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _f, _f, _f, _vp, _vp, _vp],
    "geom_stage_regularisers_bwd_f32": [_i, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _vp, _vp, _vp, _vp, _vp],
    "geom_deform_layer_fwd_f32": [_vp, _vp],
    "geom_deform_pack_weights_f32": [_i, _vp, _vp, _vp, _vp],
    "geom_deform_pack_weights_zero_f32": [_i, _vp, _vp, _vp, _vp, _i, _vp],
    "geom_deform_chain_fwd_f32": [_i, _vp, _vp, _vp],
    "geom_deform_chain_bwd_f32": [_i, _vp, _vp, _vp, _vp],
    "geom_deform_chain_fits": [_i],
    "geom_deform_layer_bwd_f32": [_vp, _vp],
    "geom_deform_layer_wide_fwd_f32": [_vp, _vp],
    "geom_deform_layer_wide_bwd_f32": [_vp, _vp],
    "geom_deform_infer_fwd_f32": [_vp, _vp],
    "geom_encoder_layer_fwd_f32": [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, ctypes.c_int64, _vp, _i, _vp, ctypes.c_int64,
                                   _vp, ctypes.c_int64, _vp, ctypes.c_int64, _vp],
    "geom_encoder_layer_bwd_f32": [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, ctypes.c_int64, _vp, ctypes.c_int64, _i, _vp,
                                   ctypes.c_int64, _vp, ctypes.c_int64, _vp, ctypes.c_int64, _vp],
    "geom_latent_l1_fwd_f32": [_i, _i, _vp, _vp, _vp, _f, _vp, _vp],
    "geom_latent_l1_bwd_f32": [_i, _i, _vp, _vp, _vp, _f, _vp, _vp, _vp],
}


class DeformFwd(ctypes.Structure):
    """struct geom_deform_fwd (include/geom_hip.h): a hidden layer of the deformation block, forward."""
    _fields_ = [("b", _i), ("nv", _i), ("c", _i), ("k", _i), ("ell_w", _i),
                ("s_in", _vp), ("bias", _vp), ("ell_col", _vp), ("ell_val", _vp),
                ("tail_col", _vp), ("tail_val", _vp),
                ("bn_w", _vp), ("bn_b", _vp), ("run_mean", _vp), ("run_var", _vp),
                ("training", _i), ("momentum", _f), ("eps", _f), ("relu", _i),
                ("res", _vp), ("res_ld", _i), ("scale", _f),
                ("z_out", _vp), ("x_out", _vp), ("save_mean", _vp), ("save_invstd", _vp),
                ("w_next", _vp), ("s_out", _vp), ("w_head", _vp), ("s_head", _vp), ("vpx", _i)]


class DeformBwd(ctypes.Structure):
    """struct geom_deform_bwd (include/geom_hip.h): a hidden layer of the deformation block, backward."""
    _fields_ = [("b", _i), ("nv", _i), ("c", _i), ("k", _i), ("ell_w", _i),
                ("dz_up", _vp), ("ell_col_t", _vp), ("ell_val_t", _vp),
                ("tail_col_t", _vp), ("tail_val_t", _vp),
                ("ds_up", _vp), ("wt_up", _vp), ("g", _vp), ("g2", _vp), ("g_ld", _i), ("g2_ld", _i),
                ("z", _vp), ("bn_w", _vp), ("bn_b", _vp), ("save_mean", _vp), ("save_invstd", _vp),
                ("relu", _i), ("has_res", _i), ("scale", _f),
                ("grad_res", _vp), ("dz", _vp), ("grad_bn_w", _vp), ("grad_bn_b", _vp), ("colsum", _vp),
                ("ds_head", _vp), ("w_head", _vp), ("x_top", _vp), ("dw_head", _vp), ("vpx", _i)]


class DeformInfer(ctypes.Structure):
    """struct geom_deform_infer (include/geom_hip.h): a hidden layer of the deformation block, eval-mode forward."""
    _fields_ = [("b", _i), ("nv", _i), ("c", _i), ("k", _i), ("ell_w", _i),
                ("s_in", _vp), ("bias", _vp), ("ell_col", _vp), ("ell_val", _vp),
                ("tail_col", _vp), ("tail_val", _vp),
                ("bn_w", _vp), ("bn_b", _vp), ("run_mean", _vp), ("run_var", _vp),
                ("eps", _f), ("relu", _i),
                ("res", _vp), ("res_ld", _i), ("scale", _f),
                ("x_out", _vp), ("w_next", _vp), ("s_out", _vp), ("w_head", _vp), ("s_head", _vp)]


class SurfaceCull(ctypes.Structure):
    """struct geom_surface_cull (include/geom_hip.h): the buffers of the culled Chamfer scan inside the surface step."""
    _fields_ = [("gt_order", ctypes.c_void_p), ("gt_index", ctypes.c_void_p), ("sample_index", ctypes.c_void_p),
                ("faces_in_order", ctypes.c_void_p)]


class SurfaceTail(ctypes.Structure):
    """struct geom_surface_tail (include/geom_hip.h): the finalize pass as extra (role) workgroups of the fused scan launch."""
    _fields_ = [("choices", ctypes.c_void_p), ("scale_sample", ctypes.c_float), ("scale_other", ctypes.c_float),
                ("want_order", ctypes.c_int), ("loss", ctypes.c_void_p), ("finalized", ctypes.c_int)]


def call(name, *args):
    """Invoke an entry point on the current stream of the current device and raise on failure."""
    code = getattr(lib(), name)(*args, stream_ptr())
    check(code, name)


def ptr(t):
    return None if t is None else t.data_ptr()

_lib = None


def _refuse_stale_library():
    """A library built from OTHER kernel sources than the ones on disk (an edit or a checkout without a rebuild) would run
    silently -- wrong numbers in every profile taken with it.  The build stamps the library with the digest of its sources;
    a mismatch is an error (GEOM_ALLOW_STALE_LIB=1 to load it anyway).  No stamp or no sources on disk: nothing to compare."""
    if os.environ.get("GEOM_ALLOW_STALE_LIB"):
        return
    try:
        from . import build
        built = build.built_digest()
        current = build.source_digest() if built else None
    except Exception:        # an installation without the sources
        return
    if built and current and built != current:
        raise RuntimeError("geometrics_amd: %s was built from other kernel sources than the ones on disk -- rebuild it with "
                           "`python -m geometrics_amd.build` (or set GEOM_ALLOW_STALE_LIB=1)" % LIB_PATH)


def lib():
    """The loaded library; raises RuntimeError when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "geometrics_amd: %s is missing -- build it with `python -m geometrics_amd.build` "
                "(hipcc, gfx950). There is no CPU/PyTorch fallback." % LIB_PATH)
        _refuse_stale_library()
        # GEOM_LIB_OVERRIDE: an instrumented build of the same sources (tools/probe: tile stamps, counters) -- never the product.
        # Said loudly: a variable that leaks into a training environment would put a probe build behind production calls.
        override = os.environ.get("GEOM_LIB_OVERRIDE")
        if override:
            import sys
            print("geometrics_amd: GEOM_LIB_OVERRIDE is set -- loading %s instead of the product library (probe builds only; "
                  "its ABI version is checked, its sources are not)" % override, file=sys.stderr)
        L = ctypes.CDLL(override or LIB_PATH)
        L.geom_abi_version.restype = _i
        L.geom_strerror.restype = ctypes.c_char_p
        L.geom_strerror.argtypes = [_i]
        if L.geom_abi_version() != ABI_VERSION:
            raise RuntimeError("geometrics_amd: libgeom_hip.so ABI %d != binding ABI %d; rebuild"
                               % (L.geom_abi_version(), ABI_VERSION))
        L.geom_pool_features_bwd_workspace_bytes.restype = ctypes.c_size_t
        L.geom_pool_features_bwd_workspace_bytes.argtypes = [_i, _i, _i, _vp]
        L.geom_segment_max_workspace_bytes.restype = ctypes.c_int64
        L.geom_segment_max_workspace_bytes.argtypes = [_i, _i, ctypes.c_int64]
        L.geom_zn_gcn_bwd_scratch_floats.restype = ctypes.c_int64
        L.geom_surface_order_words.restype = ctypes.c_int64
        L.geom_surface_order_words.argtypes = [_i, _i, _i, _i]
        L.geom_zn_gcn_relu_mask_words.restype = ctypes.c_int64
        L.geom_zn_gcn_relu_mask_words.argtypes = [_i, _i, _i, _i]
        L.geom_zn_gcn_bwd_scratch_floats.argtypes = [_i, _i, _i]
        L.geom_zn_gcn_bwd_partial_rows.restype = ctypes.c_int64
        L.geom_zn_gcn_bwd_partial_rows.argtypes = [_i, _i, _i, _i, _i]
        L.geom_dense_bwd_weight_workspace_floats.restype = ctypes.c_int64
        L.geom_dense_bwd_weight_workspace_floats.argtypes = [_i, _i, _i]
        L.geom_chamfer_nn_culled_workspace_floats.restype = ctypes.c_int64
        L.geom_chamfer_nn_culled_workspace_floats.argtypes = [_i, _i, _i]
        L.geom_nn_cull_index_floats.restype = ctypes.c_int64
        L.geom_nn_cull_index_floats.argtypes = [_i, _i]
        L.geom_tri_distance_workspace_bytes.restype = ctypes.c_size_t
        L.geom_tri_distance_workspace_bytes.argtypes = [_i, _i, _i]
        L.geom_split_bf16_kpad.restype = _i
        L.geom_split_bf16_kpad.argtypes = [_i]
        L.geom_stage_regularisers_blocks.restype = ctypes.c_int64
        L.geom_stage_regularisers_blocks.argtypes = [_i, _i, _i]
        L.geom_zn_layer_partial_rows.restype = ctypes.c_int64
        L.geom_zn_layer_partial_rows.argtypes = [_i, _i]
        L.geom_gemm_workspace_floats.restype = ctypes.c_int64
        L.geom_gemm_workspace_floats.argtypes = [_i, _i, _i]
        L.geom_adam_table_bytes.restype = ctypes.c_int64
        L.geom_adam_table_bytes.argtypes = [_i, ctypes.c_int64]
        L.geom_surface_tail_counters_offset.restype = ctypes.c_size_t
        L.geom_surface_tail_counters_offset.argtypes = [_i, _i, _i]
        for name, args in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = _i
        _lib = L
    return _lib


def declared_symbols():
    return sorted(["geom_abi_version", "geom_strerror", "geom_tri_distance_workspace_bytes",
                   "geom_zn_gcn_bwd_scratch_floats", "geom_zn_gcn_bwd_partial_rows", "geom_pool_features_bwd_workspace_bytes",
                   "geom_segment_max_workspace_bytes", "geom_zn_gcn_relu_mask_words",
                   "geom_surface_order_words",
                   "geom_dense_bwd_weight_workspace_floats", "geom_chamfer_nn_culled_workspace_floats",
                   "geom_nn_cull_index_floats", "geom_surface_tail_counters_offset", "geom_zn_layer_partial_rows",
                   "geom_gemm_workspace_floats", "geom_stage_regularisers_blocks", "geom_split_bf16_kpad",
                   "geom_adam_table_bytes"] + list(_SIGNATURES))


def check(code, what):
    if code != 0:
        msg = lib().geom_strerror(code).decode()
        raise RuntimeError("%s failed: %s (code %d)" % (what, msg, code))


def clear_hip_error():
    """Fetch-and-reset HIP's sticky last-error (e.g. after an aborted graph capture), so that the next
    launch check reports only its own failure.  Returns the stale code."""
    try:
        hip = ctypes.CDLL("libamdhip64.so")
    except OSError:
        return 0
    hip.hipGetLastError.restype = _i
    return hip.hipGetLastError()


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def require(t, name, dtype, ndim=None, last=None):
    """Validate what the reference leaves unchecked (chamfer_distance.cpp:15-27): device, dtype,
    layout.  Returns a contiguous tensor (the reference wrappers call .contiguous() too)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s must live on a HIP device (got %s); geometrics_amd has no CPU path"
                           % (name, t.device))
    if t.dtype != dtype:
        raise RuntimeError("%s must be %s (got %s)" % (name, dtype, t.dtype))
    if ndim is not None and t.dim() != ndim:
        raise RuntimeError("%s must be %d-dimensional (got shape %s)" % (name, ndim, tuple(t.shape)))
    if last is not None and t.shape[-1] != last:
        raise RuntimeError("%s must have last dimension %d (got shape %s)" % (name, last, tuple(t.shape)))
    return t.contiguous()


def same_device(*tensors):
    dev = tensors[0].device
    for t in tensors[1:]:
        if t.device != dev:
            raise RuntimeError("all tensors must be on the same device (%s vs %s)" % (dev, t.device))
    return dev

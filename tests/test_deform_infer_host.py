"""CPU: the eval-mode forward of the 192-wide deformation block (geom_deform_infer_fwd_f32, deform.serves_inference) -- no
compute on a GPU:

* the launch refuses bad arguments on the host (GEOM_EINVAL) before anything is enqueued;
* the host side of deform.serves_inference;
* tests/golden/block192_eval.npz (the reference block in eval mode, float64, tests/golden/make_block192_eval.py) pinned to the
  float64 restatement helpers.block64 with the fixture's running statistics: the tie between the new fixture and the
  restatement that test_block64_pin.py pins to the reference's training-mode results."""
import ctypes
import types

import numpy as np
import pytest
import torch

from geometrics_amd import _lib, deform, models
from deform_eval_helpers import EVAL_CASES, eval_block, eval_fixture
from helpers import block64, weighted_checksum


def _valid_args(buf):
    """A struct every field of which is acceptable, pointing into `buf` (16-byte aligned host memory: never dereferenced,
    every call below is refused before a launch)."""
    p = (ctypes.addressof(buf) + 15) & ~15
    return _lib.DeformInfer(1, 482, 192, 64, 8, p, p, p, p, None, None, p, p, p, p, 1e-5, 1, None, 0, 0.5,
                            p, p, p, None, None)


@pytest.mark.parametrize("field,value", [("b", 0), ("b", -1), ("nv", 0), ("c", 191), ("c", 384), ("k", 32), ("ell_w", 16),
                                         ("nv", 1 << 26), ("s_in", None), ("ell_col", None), ("ell_val", None),
                                         ("run_mean", None), ("run_var", None), ("s_out", None), ("res_ld", 191)])
def test_argument_rejection_without_a_gpu(field, value):
    buf = ctypes.create_string_buffer(64)
    a = _valid_args(buf)
    if field == "res_ld":
        a.res = a.s_in
    setattr(a, field, value)
    assert _lib.lib().geom_deform_infer_fwd_f32(ctypes.byref(a), None) == -1
    assert _lib.lib().geom_deform_infer_fwd_f32(None, None) == -1


def test_argument_rejection_of_inconsistent_outputs():
    buf = ctypes.create_string_buffer(64)
    L = _lib.lib()
    a = _valid_args(buf)
    a.w_next = None                          # the last layer: s_out without a product
    assert L.geom_deform_infer_fwd_f32(ctypes.byref(a), None) == -1
    a.s_out = a.x_out = None                 # ... and nothing to write at all
    assert L.geom_deform_infer_fwd_f32(ctypes.byref(a), None) == -1
    a = _valid_args(buf)
    a.w_head = a.s_in                        # a head beside a product
    a.s_head = a.s_in
    assert L.geom_deform_infer_fwd_f32(ctypes.byref(a), None) == -1
    a = _valid_args(buf)
    a.tail_col = a.s_in                      # a tail table without its values
    assert L.geom_deform_infer_fwd_f32(ctypes.byref(a), None) == -1
    a = _valid_args(buf)
    a.s_in = a.s_in + 4                      # a misaligned operand
    assert L.geom_deform_infer_fwd_f32(ctypes.byref(a), None) == -1


def test_serves_inference_host_logic():
    nv = 162
    csr = types.SimpleNamespace(ell_w=8)     # (never reached: every case below is decided before the adjacency)
    block = models.BatchMeshDeformationBlock(195, nv).eval()
    feats, pooled = torch.zeros(1, nv, 3), torch.zeros(1, nv, 192)
    with torch.no_grad():
        assert not deform.serves_inference(block, feats, pooled, csr)                  # CPU tensors
        assert not deform.serves_inference(block.train(), feats, pooled, csr)          # training mode
        narrow = models.BatchMeshDeformationBlock(51, nv, hidden=48).eval()
        assert not deform.serves_inference(narrow, feats, torch.zeros(1, nv, 48), csr)  # hidden 48
    block.eval()
    assert torch.is_grad_enabled() and not deform.serves_inference(block, feats, pooled, csr)   # gradients enabled
    deform.enabled = False
    try:
        with torch.no_grad():
            assert not deform.serves_inference(block, feats, pooled, csr)
    finally:
        deform.enabled = True


@pytest.mark.parametrize("case", EVAL_CASES)
def test_block64_reproduces_the_eval_fixture(case):
    g = eval_fixture(case)
    block = eval_block(g)
    feats, pooled = (torch.from_numpy(g[k]).double() for k in ("features", "pooled"))
    with torch.no_grad():
        f, c, _ = block64(block, feats, pooled, torch.from_numpy(g["adj"]), relu=True, running=g["running"])
    f, c = f.numpy(), c.numpy()
    rb, rv, m = (g[k].astype(np.int64) for k in ("rows_b", "rows_v", "meshes"))
    for name, got, want in (("features_rows", f[rb, rv], g["features_rows"]), ("coords", c[m], g["coords"])):
        want = want.astype(np.float64)
        err = float(np.abs(got - want).max() / np.abs(want).max())
        assert err <= 1e-6, "%s: %.2e of scale" % (name, err)
    full = {"features": f, "coords": c}
    for name, (want, scale) in zip(g["ck_names"], g["ck"]):
        got = weighted_checksum(str(name), full[str(name)])[0]
        assert abs(got - want) <= 1e-6 * scale, "%s: checksum off by %.2e of its scale" % (name, abs(got - want) / scale)

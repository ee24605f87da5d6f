"""CPU: the BatchNorm-free deformation block of the old driver (models.MeshDeformationBlock on layers.Image_ZERON_GCNGCN;
geom_deform_plain_{fwd,bwd}_f32, deform.serves_plain) -- no compute on a GPU:

* both launches refuse bad arguments on the host (GEOM_EINVAL) before anything is enqueued;
* the host side of deform.serves_plain;
* state-dict keys and shapes of the two classes (the old checkpoints');
* tests/golden/plain_block.npz (the reference's classes in float64, tests/golden/make_plain_block.py) reproduced by the
  project's classes on the CPU in float64: the separate-operator route of the class is the reference's arithmetic;
* the overlay exports both names as geometrics_amd's."""
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import deform_plain_helpers as dph
from geometrics_amd import _lib, deform, layers, models
from helpers import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _aligned(buf):
    return (ctypes.addressof(buf) + 15) & ~15


def _fwd_args(buf):
    """A struct every field of which is acceptable, pointing into `buf` (16-byte aligned host memory: never dereferenced,
    every call below is refused before a launch)."""
    p = _aligned(buf)
    return _lib.DeformPlainFwd(1, 181, 192, 64, p, p, p, p, None, None, None, 1, None, 0, 0.5, p, p, p, p, None, None)


def _bwd_args(buf):
    p = _aligned(buf)
    return _lib.DeformPlainBwd(1, 181, 192, 64, p, p, p, None, None, None, p, p, None, None, 0, 0, p, 1, 0, 0.5, None, p, p,
                               None, None, None, None)


@pytest.mark.parametrize("field,value", [("b", 0), ("b", -1), ("nv", 0), ("c", 191), ("c", 384), ("k", 32), ("nv", 1 << 26),
                                         ("s_in", None), ("ell_col", None), ("ell_val", None), ("s_out", None), ("w_next", None),
                                         ("res_ld", 191)])
def test_forward_argument_rejection_without_a_gpu(field, value):
    buf = ctypes.create_string_buffer(64)
    a = _fwd_args(buf)
    if field == "res_ld":
        a.res = a.s_in
    setattr(a, field, value)
    assert _lib.lib().geom_deform_plain_fwd_f32(ctypes.byref(a), None) == -1
    assert _lib.lib().geom_deform_plain_fwd_f32(None, None) == -1


def test_forward_rejection_of_inconsistent_operands():
    buf = ctypes.create_string_buffer(64)
    call = _lib.lib().geom_deform_plain_fwd_f32
    a = _fwd_args(buf)
    a.w_next = a.s_out = a.z_out = a.x_out = None       # nothing to write
    assert call(ctypes.byref(a), None) == -1
    a = _fwd_args(buf)
    a.w_head = a.s_head = a.s_in                         # a head beside a product
    assert call(ctypes.byref(a), None) == -1
    a = _fwd_args(buf)
    a.w_next = a.s_out = None
    a.w_head = a.s_in                                    # a head's weight without its output
    assert call(ctypes.byref(a), None) == -1
    a = _fwd_args(buf)
    a.over_col = a.over_val = a.s_in                     # an overflow list without its ptr
    assert call(ctypes.byref(a), None) == -1
    a = _fwd_args(buf)
    a.over_ptr = a.s_in                                  # ... and a ptr without its list
    assert call(ctypes.byref(a), None) == -1
    for field in ("s_in", "ell_col", "z_out", "x_out", "s_out", "w_next", "bias"):
        a = _fwd_args(buf)
        setattr(a, field, a.s_in + 4)                    # a misaligned operand
        assert call(ctypes.byref(a), None) == -1, field


@pytest.mark.parametrize("field,value", [("b", 0), ("nv", 0), ("c", 191), ("k", 32), ("nv", 1 << 26), ("dz", None), ("z", None),
                                         ("ell_col_t", None), ("ell_val_t", None), ("ds_up", None), ("wt_up", None),
                                         ("g_ld", 191), ("g2_ld", 100)])
def test_backward_argument_rejection_without_a_gpu(field, value):
    buf = ctypes.create_string_buffer(64)
    a = _bwd_args(buf)
    setattr(a, field, value)
    assert _lib.lib().geom_deform_plain_bwd_f32(ctypes.byref(a), None) == -1
    assert _lib.lib().geom_deform_plain_bwd_f32(None, None) == -1


def test_backward_rejection_of_inconsistent_operands():
    buf = ctypes.create_string_buffer(64)
    call = _lib.lib().geom_deform_plain_bwd_f32
    a = _bwd_args(buf)
    a.ds_head = a.w_head = a.dz                          # the head beside a product
    assert call(ctypes.byref(a), None) == -1
    a = _bwd_args(buf)
    a.dz_up = a.ds_up = a.wt_up = a.ell_col_t = a.ell_val_t = None      # the top layer with no gradient at all
    assert call(ctypes.byref(a), None) == -1
    a.ds_head = a.dz                                     # ... the head's gradient without its weight
    assert call(ctypes.byref(a), None) == -1
    a.w_head = a.dw_head = a.dz                          # ... its weight gradient without the layer's output
    assert call(ctypes.byref(a), None) == -1
    a = _bwd_args(buf)
    a.dw_head = a.dz                                     # partials of the head's weight gradient without the head
    assert call(ctypes.byref(a), None) == -1
    a = _bwd_args(buf)
    a.over_col_t = a.over_val_t = a.dz                   # an overflow list without its ptr
    assert call(ctypes.byref(a), None) == -1
    for field in ("dz_up", "ds_up", "wt_up", "z", "dz"):
        a = _bwd_args(buf)
        setattr(a, field, a.dz + 4)
        assert call(ctypes.byref(a), None) == -1, field


def test_serves_plain_host_logic(monkeypatch):
    nv = 42
    csr = types.SimpleNamespace(ell_w=0)     # (never reached: every case below is decided before the adjacency)
    monkeypatch.setattr(deform, "plain", True)
    block = models.MeshDeformationBlock(195)
    feats, pooled = torch.zeros(nv, 3), torch.zeros(nv, 192)
    assert not deform.serves_plain(block, feats, pooled, csr)                                   # CPU tensors
    assert not deform.serves_plain(block, feats.double(), pooled.double(), csr)                 # a foreign dtype
    narrow = models.MeshDeformationBlock(51, hidden=48)
    assert not deform.serves_plain(narrow, feats, torch.zeros(nv, 48), csr)                     # hidden 48
    monkeypatch.setattr(deform, "enabled", False)
    assert not deform.serves_plain(block, feats, pooled, csr)


def test_state_dict_keys_and_shapes():
    layer = layers.Image_ZERON_GCNGCN(40, 48)
    assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == {"weight1": (40, 48), "bias": (48,)}
    assert layer.split == 3 and "bias" not in layers.Image_ZERON_GCNGCN(4, 6, bias=False).state_dict()
    bound = 0.6 * 6.0 / np.sqrt(88)
    assert float(layer.weight1.detach().abs().max()) <= bound and float(layer.weight1.detach().abs().max()) > 0.8 * bound
    assert float(layer.bias.detach().abs().max()) <= 0.1
    block = models.MeshDeformationBlock(1155)
    want = {}
    for i in list(range(1, 14)) + [15]:
        n_in, n_out = (1155 if i == 1 else 192), (3 if i == 15 else 192)
        want["gc%d.weight1" % i], want["gc%d.bias" % i] = (n_in, n_out), (n_out,)
    assert {k: tuple(v.shape) for k, v in block.state_dict().items()} == want      # no gc14, no bn*
    assert block.hidden == 192


@pytest.mark.parametrize("case", sorted(dph.BLOCK_CASES))
def test_the_class_reproduces_the_fixture_in_float64(case):
    g = golden("plain_block")
    mesh, relu, seed = dph.BLOCK_CASES[case]
    assert (str(g[case + ".mesh"]), bool(g[case + ".relu"]), int(g[case + ".seed"])) == (mesh, relu, seed)
    adj = dph.case_adjacency(mesh, g)
    inputs = dph.case_inputs(seed, adj.shape[0], g=g, case=case)
    block = dph.fill_plain_parameters(models.MeshDeformationBlock(195), seed)
    named = dict(block.named_parameters())
    assert sorted(named) == list(g[case + ".param_names"])
    assert [float(named[n].detach().double().sum()) for n in g[case + ".param_names"]] == list(g[case + ".in_ck.params"])
    full = dph.run_block(block.double(), inputs, {"adj": torch.from_numpy(adj).double()}, relu, torch.float64)
    for name, err in dph.errors_against(g, case, full).items():
        assert err <= 1e-6, "%s: %.2e of scale" % (name, err)


def test_the_layer_reproduces_the_fixture_in_float64():
    g = golden("plain_block")
    case, mesh, seed, n_in, n_out = dph.LAYER_CASE
    adj = dph.case_adjacency(mesh, g)
    layer = dph.fill_plain_parameters(layers.Image_ZERON_GCNGCN(n_in, n_out), seed).double()
    inputs = dph.case_inputs(seed, adj.shape[0], n_in, 1, n_out, g=g, case=case)
    x = torch.from_numpy(inputs["features"]).double().requires_grad_(True)
    for given in ({"adj": torch.from_numpy(adj).double()}, torch.from_numpy(adj).double()):      # the info dict, the dense matrix
        x.grad = layer.weight1.grad = layer.bias.grad = None
        y = layer(x, given, torch.nn.functional.relu)
        (y * torch.from_numpy(inputs["g_features"]).double()).sum().backward()
        for name, got in (("out", y), ("grad.input", x.grad), ("grad.weight1", layer.weight1.grad), ("grad.bias", layer.bias.grad)):
            want = g["%s.%s" % (case, name)].astype(np.float64)
            err = float(np.abs(got.detach().numpy() - want).max() / np.abs(want).max())
            assert err <= 1e-6, "%s: %.2e of scale" % (name, err)


def test_the_overlay_exports_both_classes(tmp_path):
    (tmp_path / "models.py").write_text("class MeshDeformationBlock:\n    pass\n")
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "import models, layers, geometrics_amd.models as m, geometrics_amd.layers as l\n"
            "assert models.MeshDeformationBlock is m.MeshDeformationBlock\n"
            "assert layers.Image_ZERON_GCNGCN is l.Image_ZERON_GCNGCN\n" % (os.path.join(ROOT, "overlay"), ROOT, str(tmp_path)))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=120)

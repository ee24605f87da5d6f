"""CPU: the batched mesh encoder's names and shapes are the reference's (tests/golden/batch_mesh_encoder.npz records its
state_dict), the four entry points of csrc/encoder_stack.hip validate their arguments before any launch, and the encoder and the
latent loss refuse CPU tensors like every other operator."""
import pytest
import torch

from helpers import golden
from geometrics_amd import _lib

I64 = 8      # any non-null address: validation never dereferences


def test_state_dict_keys_and_shapes_are_the_reference_s():
    from geometrics_amd import models
    g = golden("batch_mesh_encoder")
    want = [(str(k), tuple(int(d) for d in s if d)) for k, s in zip(g["state_keys"], g["state_shapes"])]
    enc = models.BatchMeshEncoder(50)
    assert [(k, tuple(t.shape)) for k, t in enc.state_dict().items()] == want
    assert len(want) == 34 and want[0] == ("h1.weight", (3, 60)) and want[-2] == ("reduce.weight_Ws.0", (300, 50))


def _fwd(L, b=1, nv=4, c=8, k=0, n=8, csr=I64, s=I64, lds=None, bias=None, act=2, w=I64, ldw=None, out=I64, ldo=None, x=None, ldx=None):
    csr3 = (csr, csr, csr)
    return L.geom_encoder_layer_fwd_f32(b, nv, c, k, n, *csr3, s, c if lds is None else lds, bias, act, w, n if ldw is None else ldw,
                                        out, n if ldo is None else ldo, x, c if ldx is None else ldx, None)


def _bwd(L, b=1, nv=4, c=8, k=0, n=8, csr=I64, g=I64, ldg=None, x=I64, ldx=None, act=2, w=I64, ldw=None, out=I64, ldo=None, t=None,
         ldt=None):
    csr3 = (csr, csr, csr)
    return L.geom_encoder_layer_bwd_f32(b, nv, c, k, n, *csr3, g, c if ldg is None else ldg, x, c if ldx is None else ldx, act, w,
                                        c if ldw is None else ldw, out, n if ldo is None else ldo, t, c if ldt is None else ldt, None)


@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_layer_entry_points_refuse_bad_arguments_before_any_launch(call):
    L = _lib.lib()
    for size in ("b", "nv", "c", "k", "n"):
        assert call(L, **{size: -1}) == -1, size                      # negative sizes
    assert call(L, c=8, k=9) == -1                                    # k > c
    assert call(L, c=400, k=33, n=4) == _lib.EUNSUPPORTED             # the aggregated columns leave the first k-stage
    assert call(L, c=400, k=32, n=4, out=None) == -1                  # (k = 32 itself is served: it reaches the pointer checks)
    assert call(L, act=3) == -1
    assert call(L, out=None) == -1                                    # null pointers
    assert call(L, w=None) == -1
    assert call(L, k=2, csr=None) == -1                               # an adjacency is needed as soon as a column is aggregated
    assert call(L, ldw=7) == -1                                       # pitches below the width (c = n = 8)
    assert call(L, ldo=7) == -1
    assert call(L, b=0) == 0 and call(L, n=0) == 0                    # nothing to do
    if call is _fwd:
        assert call(L, s=None) == -1
        assert call(L, lds=7) == -1
        assert call(L, x=I64, ldx=7) == -1
    else:
        assert call(L, g=None) == -1
        assert call(L, x=None) == -1                                  # the saved output, for act'
        assert call(L, ldg=7) == -1
        assert call(L, ldx=7) == -1
        assert call(L, t=I64, ldt=7) == -1


def test_latent_loss_entry_points_refuse_bad_arguments_before_any_launch():
    L = _lib.lib()
    assert L.geom_latent_l1_fwd_f32(-1, 50, I64, I64, I64, .0005, I64, None) == -1
    assert L.geom_latent_l1_fwd_f32(2, -1, I64, I64, I64, .0005, I64, None) == -1
    assert L.geom_latent_l1_fwd_f32(2, 50, I64, I64, I64, .0005, None, None) == -1
    for missing in range(3):
        ptrs = [I64, I64, I64]
        ptrs[missing] = None
        assert L.geom_latent_l1_fwd_f32(2, 50, *ptrs, .0005, I64, None) == -1
        assert L.geom_latent_l1_bwd_f32(2, 50, *ptrs, .0005, I64, I64, None) == -1
    assert L.geom_latent_l1_bwd_f32(-1, 50, I64, I64, I64, .0005, I64, I64, None) == -1
    assert L.geom_latent_l1_bwd_f32(2, 50, I64, I64, I64, .0005, None, I64, None) == -1
    assert L.geom_latent_l1_bwd_f32(2, 50, I64, I64, I64, .0005, I64, None, None) == -1
    assert L.geom_latent_l1_bwd_f32(0, 50, None, None, None, .0005, None, None, None) == 0   # nothing to do


def test_encoder_and_latent_loss_refuse_cpu_tensors():
    from geometrics_amd import encoder, models, utils
    lat = torch.zeros(2, 50)
    with pytest.raises(RuntimeError, match="HIP device"):
        utils.latent_loss(lat, lat, torch.ones(2))
    enc = models.BatchMeshEncoder(50).requires_grad_(False)
    for on in (False, True):                                          # whichever route the switch selects
        was, encoder.enabled = encoder.enabled, on
        try:
            with pytest.raises(RuntimeError, match="HIP device"):
                enc(torch.zeros(2, 4, 3), torch.eye(4))
        finally:
            encoder.enabled = was
    assert enc.last_route == "separate"                               # a CPU input never selects the fused launches

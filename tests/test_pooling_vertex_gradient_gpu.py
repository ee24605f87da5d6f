"""-m gpu: the pooling's hand-derived vertex-position gradient (csrc/pooling.hip: pool_bwd_verts_body's per-chunk sums,
pool_bwd_verts_finish_body's fixed-order sum and closed-form chain), its projection and its bilinear weights, element by element
against the float64 restatement oracle/ref_ops.py pool_features / pool_vertex_gradient (pinned on the host against the
reference's fixture by tests/test_oracle_pin.py).  The restatement gets the fp32 cameras utils.batch_camera_info returned.

Bounds (helpers.pool_vertex_gradient_close): |error| <= 8 eps * (the element's term mass) + 1 texel-coordinate ulp through every
term (eps * dim^2 * |g_c| * sum |texel| * |J|: the weights are differences of the fp32 xs * dim and a whole number, so their
absolute rounding does not shrink with the weight).  Vertices within 1e-3 texels of a texel line are left out -- the gradient
jumps across a line, the fp32 texel coordinate is within 1e-5 of the float64 one --, at most 2 % of a case's vertices (asserted;
the inputs below leave out 1 / 202, 1 / 202, 3 / 324 and 6 / 1446).  A single dropped or misplaced channel term is about 1e-3
of a row's mass against about 4 eps dim <= 1.4e-5 of it for the bound.

What the bounds are judged against -- the restatement's OWN fp32 run (the same expressions in torch fp32 on the host, autograd)
on the same inputs, worst element as a share of its bound:
    ragged four maps 0.071, ragged two maps 0.087, 2 x 1280 channels 0.017, training shape 0.066 (0.078 / 0.113 / 0.023 / 0.075
    of the floor part alone); the reference's fp32 run stored in the pooling_v162 fixture: 0.49.
Measured margins of the kernel (GEOM_MARGIN_LOG, MI355X), same order:
    0.081, 0.083 (the same with the gradient pitched and in the vertices-only launch), 0.015, 0.077 (pitched: the same);
    the 40-chunk launch on device-drawn maps (test_ops_parity_gpu.py): 0.021.
Projection and weights: the restatement's fp32 P (identity maps pooled) against its float64 P reaches 1.175 eps * dim on the
kept vertices of these inputs (ragged: 0.85 at 13 x 13; training: 1.175 at 7 x 7), so the kernel's bar is 4 x that =
POOL_P_ULPS = 4.7 eps * dim; the kernel reaches 0.90 (ragged) and 1.02 (training)."""
import numpy as np
import pytest
import torch

from helpers import POOL_NEAR, pool_vertex_gradient_close
from geometrics_amd import meshgen, ops, utils
from oracle import ref_ops

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)
POOL_P_ULPS = 4.7


# ---------------------------------------------------------------- inputs (host tensors: what the host-side margins above are measured on)
def ragged_inputs():
    """The vertices and cameras of test_pooling_at_ragged_shapes_per_element: 101 vertices (no multiple of the 64-vertex tile)
    at three radii, the outer one outside the image for some cameras (clamped on one axis or on both)."""
    V, _ = meshgen.icosphere(1)
    V = np.concatenate([V, 0.5 * V, 2.5 * V], 0)[:101]
    return torch.from_numpy(meshgen.jittered_batch(V, 2)), torch.tensor([[35.0, 20.0, 1.2], [250.0, -30.0, 0.8]])


def training_inputs():
    """Those of test_pooling_map_gradient_per_element_at_the_training_shape: 482 vertices, three cameras."""
    V, _ = meshgen.icosphere(2)
    V = np.concatenate([V, 0.6 * V, 0.3 * V], 0)[:482]
    return torch.from_numpy(meshgen.jittered_batch(V, 3)), torch.tensor([[35.0, 20.0, 1.2], [200.0, -10.0, 1.0], [310.0, 45.0, 1.4]])


def wide_inputs():
    """Those of test_pooling_with_more_channel_chunks_than_grid_slices: icosphere(2), two cameras."""
    V, _ = meshgen.icosphere(2)
    return torch.from_numpy(meshgen.jittered_batch(V, 2)), torch.tensor([[35.0, 20.0, 1.2], [60.0, 30.0, 1.0]])


def maps_and_gradient(seed, verts, chans, dims):
    """Seeded N(0, 1) maps [b, c, d, d] and output gradient [b, nv, sum c] (host generator: the same on every machine)."""
    gen = torch.Generator().manual_seed(seed)
    b, nv = verts.shape[:2]
    maps = [torch.randn(b, c, d, d, generator=gen) for c, d in zip(chans, dims)]
    return maps, torch.randn(b, nv, sum(chans), generator=gen)


RAGGED_SHAPES = {"four_maps": ((70, 130, 260, 5), (5, 9, 40, 1)), "two_maps": ((3, 64), (2, 13))}
TRAINING_SHAPE = ((64, 128, 256, 512), (56, 28, 14, 7))
WIDE_SHAPE = ((1280, 1280), (14, 7))


# ---------------------------------------------------------------- the kernel's side
def kernel_vertex_gradient(gpu, monkeypatch, verts, img_info, maps, grad_out, headroom, maps_want_grad):
    """verts.grad of utils.batched_pooling(headroom=...) on the device for the output gradient `grad_out`, handed to the backward
    as the trailing columns of a buffer `headroom` columns wider (so the kernel reads it pitched, as in the training step) -- the
    row pitch the backward launch was given is checked.  Returns (the gradient, the fp32 cameras used)."""
    cam_mat, cam_pos = utils.batch_camera_info(img_info.to(gpu))
    v = verts.to(gpu).requires_grad_(True)
    m = [t.to(gpu).requires_grad_(maps_want_grad) for t in maps]
    feats = utils.batched_pooling(m, v, (cam_mat, cam_pos), headroom=headroom)
    ctot = grad_out.shape[2]
    wide = torch.zeros(grad_out.shape[0], grad_out.shape[1], headroom + ctot, device=gpu)
    wide[..., headroom:] = grad_out.to(gpu)
    pitches, call = [], ops._lib.call

    def recording_call(name, *args):
        if name == "geom_pool_features_bwd_ld_f32":
            pitches.append(int(args[10]))                    # grad_ld (0 = the pooled width)
        return call(name, *args)

    monkeypatch.setattr(ops._lib, "call", recording_call)
    got = torch.autograd.grad(feats, [v] + (m if maps_want_grad else []), wide[..., headroom:])
    monkeypatch.setattr(ops._lib, "call", call)
    assert pitches == [headroom + ctot if headroom else 0]
    return got[0], (cam_mat, cam_pos)


@pytest.mark.parametrize("maps_want_grad", (True, False), ids=("with_maps", "verts_only"))
@pytest.mark.parametrize("headroom", (0, 7))
@pytest.mark.parametrize("shape", sorted(RAGGED_SHAPES))
def test_vertex_gradient_at_ragged_shapes(gpu, monkeypatch, shape, headroom, maps_want_grad):
    """Maps of more than 64 channels (several per-chunk sums per vertex, a partial last chunk each: 70 / 130 / 260 channels), 3
    and 5 channels (fewer than a workgroup has waves), 1 x 1 and 2 x 2 maps, 101 vertices, vertices clamped on one axis only and
    on both (exactly zero rows), the gradient contiguous and pitched, and the launch in which only the vertices want a gradient
    (no binning workgroups, no gather slices: the finish role is grid.z slice 0)."""
    chans, dims = RAGGED_SHAPES[shape]
    verts, img_info = ragged_inputs()
    maps, grad_out = maps_and_gradient(32, verts, chans, dims)
    got, cams = kernel_vertex_gradient(gpu, monkeypatch, verts, img_info, maps, grad_out, headroom, maps_want_grad)
    r = pool_vertex_gradient_close(got, maps, verts, *cams, grad_out,
                                   "pooling verts.grad ragged %s headroom %d %s" % (shape, headroom, "maps" if maps_want_grad else "verts only"))
    # (24 / 25 rows of the float64 gradient are all zero; one of the 24 sits 8.7e-4 from a texel line and is left out)
    assert r["zero_rows"] >= 24 and r["zero_checked"] >= 23 and r["live_rows"] > 170, r


def test_vertex_gradient_with_more_chunks_than_grid_slices(gpu, monkeypatch):
    """Two maps of 1280 channels = 40 chunks of 64: a workgroup of the first 8 grid slices walks two chunks and leaves ONE sum."""
    verts, img_info = wide_inputs()
    maps, grad_out = maps_and_gradient(12, verts, *WIDE_SHAPE)
    got, cams = kernel_vertex_gradient(gpu, monkeypatch, verts, img_info, maps, grad_out, 0, True)
    r = pool_vertex_gradient_close(got, maps, verts, *cams, grad_out, "pooling verts.grad 2 x 1280 channels")
    assert r["live_rows"] > 300, r


@pytest.mark.parametrize("headroom", (0, 195))
def test_vertex_gradient_at_the_training_shape(gpu, monkeypatch, headroom):
    """482 vertices, three meshes, the four VGG maps (15 chunks), the gradient contiguous and as the trailing 960 columns of the
    1155-wide buffer of the training step."""
    verts, img_info = training_inputs()
    maps, grad_out = maps_and_gradient(31, verts, *TRAINING_SHAPE)
    got, cams = kernel_vertex_gradient(gpu, monkeypatch, verts, img_info, maps, grad_out, headroom, True)
    r = pool_vertex_gradient_close(got, maps, verts, *cams, grad_out, "pooling verts.grad training shape headroom %d" % headroom)
    assert r["live_rows"] > 1400, r


def test_vertex_gradient_is_bit_reproducible(gpu):
    """The per-chunk sums are added in chunk order, whatever order the workgroups finished in: two backward calls, same bits
    (40 chunks on 32 grid slices, and the training shape)."""
    for (verts, img_info), shape, seed in ((wide_inputs(), WIDE_SHAPE, 12), (training_inputs(), TRAINING_SHAPE, 31)):
        maps, grad_out = maps_and_gradient(seed, verts, *shape)
        v = verts.to(gpu).requires_grad_(True)
        m = [t.to(gpu).requires_grad_(True) for t in maps]
        feats = utils.batched_pooling(m, v, img_info.to(gpu))
        g = grad_out.to(gpu)
        first = torch.autograd.grad(feats, [v] + m, g, retain_graph=True)[0]
        again = torch.autograd.grad(feats, [v] + m, g)[0]
        assert torch.equal(first, again)
        assert float(first.abs().max()) > 0


# ---------------------------------------------------------------- projection and weights
def weights_against_float64(P, verts, cam_mat, cam_pos, dim, keep):
    """P [b, nv, dim * dim] -- identity maps pooled by an fp32 evaluation -- against the restatement's float64 P on the kept
    vertices: the worst |difference| in texel-coordinate ulps (eps * dim); an entry that is zero in one and not in the other is
    a failure whatever its size."""
    b = verts.shape[0]
    eye = torch.eye(dim * dim, dtype=torch.float64).view(1, dim * dim, dim, dim).expand(b, -1, -1, -1)
    exact = ref_ops.pool_features([eye], verts.double(), cam_mat.double(), cam_pos.double())[torch.from_numpy(keep)]
    P = P.double().cpu()[torch.from_numpy(keep)]
    assert bool(((P == 0) == (exact == 0)).all()), "%d x %d: a weight is zero on one side only" % (dim, dim)
    return float((P - exact).abs().max()) / (EPS * dim)


@pytest.mark.parametrize("case", ("ragged", "training"))
def test_projection_and_weights_against_float64(gpu, case):
    """The kernel's P (pooling identity maps: channel t = the one-hot map of texel t) against the restatement's float64 P, per
    element, on the vertices at least 1e-3 from every texel line of the case's maps: which texels a vertex reads and with which
    weights.  Bound POOL_P_ULPS * eps * dim = 4 x the worst the restatement's own fp32 run reaches on these inputs (1.175)."""
    (verts, img_info), dims = (ragged_inputs(), (5, 9, 40, 1, 2, 13)) if case == "ragged" else (training_inputs(), TRAINING_SHAPE[1])
    cam_mat, cam_pos = utils.batch_camera_info(img_info.to(gpu))
    b, nv = verts.shape[:2]
    planes = [torch.zeros(b, 1, d, d) for d in dims]
    near = ref_ops.pool_vertex_gradient(planes, verts, cam_mat.cpu(), cam_pos.cpu(), torch.zeros(b, nv, len(dims)))[3]
    keep = near >= POOL_NEAR
    assert (~keep).mean() <= 0.02
    worst = 0.0
    for d in dims:
        eye = torch.eye(d * d, device=gpu).view(1, d * d, d, d).expand(b, -1, -1, -1).contiguous()
        P = utils.batched_pooling([eye], verts.to(gpu), (cam_mat, cam_pos))
        worst = max(worst, weights_against_float64(P, verts, cam_mat.cpu(), cam_pos.cpu(), d, keep))
    from helpers import log_margin
    assert log_margin("pooling P %s (eps * dim)" % case, worst, POOL_P_ULPS), "the kernel's weights are %.2f eps * dim off" % worst

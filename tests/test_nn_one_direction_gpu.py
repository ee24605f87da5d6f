"""-m gpu: GEOM_FLAG_NN_SAMPLES_ONLY -- the Chamfer scan of the surface step without the direction the one-sided loss never
reads (the nearest sampled point of every gt point: sq_gt / idx_p).  Every comparison is torch.equal: leaving half of the
Chamfer jobs out must change no bit of anything else, on every route the scan can take --

  fused, brute-force Chamfer tiles   8 x the 162-vertex icosphere (320 faces), 2048 gt points, 1000 samples: 8 x 32 = 256 query
                                     tiles is the smallest count that fuses; 1000 samples leave a ragged last query tile and a
                                     ragged last target group
  separate launches                  2 meshes, 300 gt points, 200 samples; and geom_chamfer_nn_f32 alone, n != m both ways
  fused, culled tiles + finalize     8 meshes, 1985 gt points (256 tiles), 2048 sorted samples from the prepare call: the tiles'
  roles                              completion counters and the roles' expectations must follow the halved job count
                                     (an ordinary run: no role is made to give up)
  python                             utils.batch_point_to_surface drops the direction exactly when nothing reads it.

The host-only refusals are in tests/test_nn_one_direction_host.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from geometrics_amd import _lib as L
from geometrics_amd import layers, meshgen, ops, optim, utils
from geometrics_amd.chamfer_distance import chamfer_nn
from geometrics_amd.tri_distance import face_order, faces_in_order

pytestmark = pytest.mark.gpu

ONE = L.FLAG_NN_SAMPLES_ONLY
SCAN_OUTPUTS = ("sq_pred", "idx_g", "tri_dist", "option", "index", "sq", "closest", "weights")
SENTINEL = -7


@functools.lru_cache(maxsize=None)
def _scene(b, n_gt, num, seed=21):
    """b jittered 162-vertex icospheres, a gt cloud and one set of draws with their sampled points."""
    gpu = torch.device("cuda:0")
    V, Fc = meshgen.icosphere(2)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu).contiguous()
    verts, faces, gt = to(meshgen.jittered_batch(V, b)), to(Fc), to(meshgen.gt_cloud(b, n_gt))
    ops.manual_seed(seed)
    choices, u, v, points = ops.draw_samples(verts, faces, num, with_points=True)
    return dict(b=b, n_gt=n_gt, num=num, verts=verts, faces=faces, gt=gt, tri_order=face_order(verts, faces), choices=choices, u=u,
                v=v, points=points)


def _records(scratch, b, nf, cap):
    """The gradient records' words of an order scratch (csrc/surface_layout.h: behind off | seg | pface | slot, padded to 4)."""
    first = (b * (nf + 1) + 3 * b * cap + 3) & ~3
    return scratch[first:first + b * cap * 8]


def _scan(s, flags, with_scratch, null_gt_side=False, tri=True):
    """One geom_surface_scan_f32 on the scene's draws: (return code, outputs).  sq_gt / idx_p start as a sentinel."""
    b, n_gt, num = s["b"], s["n_gt"], s["num"]
    verts, faces = s["verts"], s["faces"]
    gpu, lib, nv, nf = verts.device, L.lib(), verts.shape[1], faces.shape[0]
    f32, i32 = dict(dtype=torch.float32, device=gpu), dict(dtype=torch.int32, device=gpu)
    ws_bytes = lib.geom_tri_distance_workspace_bytes(b, n_gt, nf)
    o = dict(sq_gt=torch.full((b, n_gt), float(SENTINEL), **f32), idx_p=torch.full((b, n_gt), SENTINEL, **i32),
             sq_pred=torch.empty(b, num, **f32), idx_g=torch.empty(b, num, **i32), tri_dist=torch.empty(b, n_gt, **f32),
             option=torch.empty(b, n_gt, **i32), index=torch.empty(b, n_gt, **i32), sq=torch.empty(b, n_gt, **f32),
             closest=torch.empty(b, n_gt, 3, **f32), weights=torch.empty(b, n_gt, 3, **f32), ws=torch.zeros(ws_bytes // 4, **f32),
             scratch=torch.zeros(lib.geom_surface_order_words(b, nf, num, n_gt), **i32))
    wrote = ctypes.c_int(-1)
    tri_args = (nv, verts.data_ptr(), nf, faces.data_ptr(), s["tri_order"].data_ptr(), o["tri_dist"].data_ptr(), o["option"].data_ptr(),
                o["index"].data_ptr(), o["sq"].data_ptr(), o["closest"].data_ptr(), o["weights"].data_ptr()) if tri else \
               (nv, None, nf, None, None, None, None, None, None, None, None)
    rc = lib.geom_surface_scan_f32(b, n_gt, s["gt"].data_ptr(), num, s["points"].data_ptr(),
                                   None if null_gt_side else o["sq_gt"].data_ptr(), None if null_gt_side else o["idx_p"].data_ptr(),
                                   o["sq_pred"].data_ptr(), o["idx_g"].data_ptr(), *tri_args, s["u"].data_ptr(), s["v"].data_ptr(),
                                   3000.0 / (b * num), 3000.0 / (b * n_gt), o["scratch"].data_ptr() if with_scratch else None, flags,
                                   o["ws"].data_ptr(), ws_bytes, ctypes.byref(wrote), None, None, L.stream_ptr())
    torch.cuda.synchronize()
    o["records_written"] = wrote.value
    return rc, o


def _assert_same_scan(s, flagged, both, with_scratch):
    b, n_gt, num, nf = s["b"], s["n_gt"], s["num"], s["faces"].shape[0]
    for k in SCAN_OUTPUTS:
        assert torch.equal(flagged[k], both[k]), k
    assert flagged["records_written"] == both["records_written"]
    assert torch.equal(_records(flagged["scratch"], b, nf, num + n_gt), _records(both["scratch"], b, nf, num + n_gt))
    assert torch.equal(flagged["scratch"], both["scratch"])
    # the gt points' side: filled without the flag, never touched with it
    assert int((both["idx_p"] >= 0).all()) and int((both["idx_p"] < num).all()) and float(both["sq_gt"].min()) >= 0
    assert bool((flagged["idx_p"] == SENTINEL).all()) and bool((flagged["sq_gt"] == float(SENTINEL)).all())
    d1, i1, d2, i2 = chamfer_nn(s["gt"], s["points"])
    assert torch.equal(flagged["sq_pred"], d2) and torch.equal(flagged["idx_g"], i2)
    assert torch.equal(both["sq_gt"], d1) and torch.equal(both["idx_p"], i1)


@pytest.mark.parametrize("with_scratch", [True, False], ids=["records", "no-scratch"])
def test_fused_scan_with_the_flag_equals_the_scan_without(gpu, with_scratch):
    s = _scene(8, 2048, 1000)
    rc_both, both = _scan(s, 0, with_scratch)
    rc_one, flagged = _scan(s, ONE, with_scratch)
    assert rc_both == 0 and rc_one == 0
    assert both["records_written"] == int(with_scratch)          # the fused route writes the records where it has a scratch
    if with_scratch:
        assert bool(_records(both["scratch"], 8, 320, 3048).any())
    _assert_same_scan(s, flagged, both, with_scratch)
    rc_null, nulled = _scan(s, ONE, with_scratch, null_gt_side=True)
    assert rc_null == 0
    for k in SCAN_OUTPUTS + ("scratch",):
        assert torch.equal(nulled[k], both[k]), k


def test_separate_launches_with_the_flag_equal_those_without(gpu):
    s = _scene(2, 300, 200)
    rc_both, both = _scan(s, 0, True)
    rc_one, flagged = _scan(s, ONE, True)
    assert rc_both == 0 and rc_one == 0 and both["records_written"] == 0          # below 256 query tiles: not the fused launch
    _assert_same_scan(s, flagged, both, True)
    assert _scan(s, ONE, True, null_gt_side=True)[0] == 0


@pytest.mark.parametrize("n,m", [(300, 200), (200, 300), (1000, 64), (65, 1000)])
@pytest.mark.parametrize("fma", [False, True], ids=["unfused", "fma"])
def test_chamfer_nn_alone_with_the_flag(gpu, n, m, fma):
    b = 3
    g = torch.Generator().manual_seed(n * 7 + m)
    x, y = torch.rand(b, n, 3, generator=g).to(gpu), torch.rand(b, m, 3, generator=g).to(gpu)
    flags = L.FLAG_NN_FMA if fma else 0
    f32, i32 = dict(dtype=torch.float32, device=gpu), dict(dtype=torch.int32, device=gpu)
    d1, i1, d2, i2 = chamfer_nn(x, y, flags)
    r1, j1 = torch.full((b, n), float(SENTINEL), **f32), torch.full((b, n), SENTINEL, **i32)
    r2, j2 = torch.empty(b, m, **f32), torch.empty(b, m, **i32)
    lib = L.lib()
    assert lib.geom_chamfer_nn_f32(b, n, x.data_ptr(), m, y.data_ptr(), r1.data_ptr(), j1.data_ptr(), r2.data_ptr(), j2.data_ptr(),
                                   flags | ONE, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(r2, d2) and torch.equal(j2, i2)
    assert bool((r1 == float(SENTINEL)).all()) and bool((j1 == SENTINEL).all())
    r2.fill_(-1), j2.fill_(-1)
    assert lib.geom_chamfer_nn_f32(b, n, x.data_ptr(), m, y.data_ptr(), None, None, r2.data_ptr(), j2.data_ptr(), flags | ONE,
                                   L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(r2, d2) and torch.equal(j2, i2)
    assert int(i1.max()) < m and int(i2.max()) < n          # (the reference call did fill both sides)


def test_refusals_on_real_buffers(gpu):
    """The same calls are accepted without the flag (or without the fault): the flag alone makes them GEOM_EINVAL."""
    fused, small = _scene(8, 2048, 1000), _scene(2, 300, 200)
    for s in (fused, small):
        assert _scan(s, 0, True, tri=False)[0] == 0
        assert _scan(s, ONE, True, tri=False)[0] == -1                                   # the two-sided records need both directions
        assert _scan(s, L.FLAG_REF_TAIL_TRUNC, True)[0] == 0
        assert _scan(s, ONE | L.FLAG_REF_TAIL_TRUNC, True)[0] == -1                      # the truncation mode keeps its own kernels
        assert _scan(s, 0, True, null_gt_side=True)[0] == -1                              # NULL sq_gt / idx_p only under the flag
    x = small["gt"]
    out = lambda n, dt: torch.empty(2, n, dtype=dt, device=x.device)
    r1, j1, r2, j2 = out(300, torch.float32), out(300, torch.int32), out(200, torch.float32), out(200, torch.int32)
    nn = lambda a, b_, flags: L.lib().geom_chamfer_nn_f32(2, 300, x.data_ptr(), 200, small["points"].data_ptr(), a, b_, r2.data_ptr(),
                                                          j2.data_ptr(), flags, L.stream_ptr())
    assert nn(r1.data_ptr(), j1.data_ptr(), ONE | L.FLAG_REF_TAIL_TRUNC) == -1
    assert nn(None, None, 0) == -1 and nn(None, j1.data_ptr(), 0) == -1
    assert nn(r1.data_ptr(), j1.data_ptr(), L.FLAG_REF_TAIL_TRUNC) == 0
    torch.cuda.synchronize()


# ---- the culled route with the finalize roles: the harness of tests/test_surface_route_gpu.py at its smallest fusing size -----
def _culled_step(flags):
    b, num, n_gt = 8, 2048, 1985
    gpu = torch.device("cuda:0")
    V, Fc = meshgen.icosphere(2)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu).contiguous()
    verts, faces, gt = to(meshgen.jittered_batch(V, b)), to(Fc), to(meshgen.gt_cloud(b, n_gt))
    tri_order, in_order, gi = face_order(verts, faces), faces_in_order(verts, faces), ops.GtIndex(gt)
    lib, nv, nf = L.lib(), verts.shape[1], faces.shape[0]
    f32, i32 = dict(dtype=torch.float32, device=gpu), dict(dtype=torch.int32, device=gpu)
    ws_bytes = lib.geom_tri_distance_workspace_bytes(b, n_gt, nf)
    o = dict(sq_gt=torch.full((b, n_gt), float(SENTINEL), **f32), idx_p=torch.full((b, n_gt), SENTINEL, **i32),
             sq_pred=torch.empty(b, num, **f32), idx_g=torch.empty(b, num, **i32), tri_dist=torch.empty(b, n_gt, **f32),
             option=torch.empty(b, n_gt, **i32), index=torch.empty(b, n_gt, **i32), sq=torch.empty(b, n_gt, **f32),
             closest=torch.empty(b, n_gt, 3, **f32), weights=torch.empty(b, n_gt, 3, **f32), ws=torch.zeros(ws_bytes // 4, **f32),
             scratch=torch.zeros(lib.geom_surface_order_words(b, nf, num, n_gt), **i32), loss=torch.zeros((), **f32),
             grad_verts=torch.empty(b, nv, 3, **f32))
    choices = torch.empty(b, num, dtype=torch.int64, device=gpu)
    u, v, points = torch.empty(b, num, **f32), torch.empty(b, num, **f32), torch.empty(b, num, 3, **f32)
    s_index = torch.zeros(max(int(lib.geom_nn_cull_index_floats(b, num)), 4), **f32)
    ops.manual_seed(21)
    prepared = ctypes.c_int(-1)
    draw_cull = L.SurfaceCull(None, None, s_index.data_ptr(), in_order.data_ptr())
    L.check(lib.geom_surface_prepare_f32(b, nv, verts.data_ptr(), nf, faces.data_ptr(), num, ops._rng_state(gpu).data_ptr(),
                                         choices.data_ptr(), u.data_ptr(), v.data_ptr(), points.data_ptr(), n_gt, tri_order.data_ptr(),
                                         0, o["ws"].data_ptr(), ws_bytes, ctypes.byref(prepared), ctypes.byref(draw_cull),
                                         L.stream_ptr()), "geom_surface_prepare_f32")
    assert prepared.value == 3          # triangle records + the sorted samples' index: the culled tiles are reachable
    scan_cull = L.SurfaceCull(gi.order.data_ptr(), gi.index.data_ptr(), s_index.data_ptr(), None)
    coef_s, coef_o = 3000.0 / (b * num), 3000.0 / (b * n_gt)
    tail = L.SurfaceTail(choices.data_ptr(), coef_s, coef_o, 1, o["loss"].data_ptr(), -1)
    wrote = ctypes.c_int(-1)
    L.check(lib.geom_surface_scan_f32(b, n_gt, gt.data_ptr(), num, points.data_ptr(), o["sq_gt"].data_ptr(), o["idx_p"].data_ptr(),
                                      o["sq_pred"].data_ptr(), o["idx_g"].data_ptr(), nv, verts.data_ptr(), nf, faces.data_ptr(),
                                      tri_order.data_ptr(), o["tri_dist"].data_ptr(), o["option"].data_ptr(), o["index"].data_ptr(),
                                      o["sq"].data_ptr(), o["closest"].data_ptr(), o["weights"].data_ptr(), u.data_ptr(), v.data_ptr(),
                                      coef_s, coef_o, o["scratch"].data_ptr(), flags | L.FLAG_TRI_WS_READY, o["ws"].data_ptr(),
                                      ws_bytes, ctypes.byref(wrote), ctypes.byref(scan_cull), ctypes.byref(tail), L.stream_ptr()),
            "geom_surface_scan_f32")
    vf_ptr, vf_item = ops.vertex_faces(faces, nv)
    L.call("geom_surface_gather_f32", b, nv, nf, vf_ptr.data_ptr(), vf_item.data_ptr(), num, n_gt, 1, o["scratch"].data_ptr(), None,
           o["grad_verts"].data_ptr())
    torch.cuda.synchronize()
    o.update(finalized=tail.finalized, records_written=wrote.value, points=points, gt=gt)
    return o


def _without_arrival_slots(scratch, b, nf, cap):
    """The order scratch without the lower halves of its `slot` words.  Those are each point's ARRIVAL slot inside its face, an
    LDS atomic of the in-launch roles (csrc/finalize_body.h: bin_point) and their working memory only: two runs of the same
    call without the flag differ in ~6000 of the 32 264 words there (measured on an MI355X), in nothing else.  Everything the
    backward reads -- offsets, ordered ids, faces, run positions (the upper halves), records, status words -- is compared."""
    out = scratch.clone()
    first = b * (nf + 1) + 2 * b * cap
    out[first:first + b * cap] &= ~0xffff
    return out


def test_culled_tiles_and_finalize_roles_with_the_flag(gpu):
    both, flagged = _culled_step(0), _culled_step(ONE)
    b, n_gt, nf, cap = 8, 1985, 320, 2048 + 1985
    assert both["finalized"] == 1 and flagged["finalized"] == 1
    assert both["records_written"] == 1 and flagged["records_written"] == 1
    assert torch.equal(both["points"], flagged["points"])          # (the same draws)
    assert bool(torch.isfinite(both["loss"])) and float(both["loss"]) > 0
    assert torch.equal(flagged["loss"], both["loss"])
    for k in SCAN_OUTPUTS:
        assert torch.equal(flagged[k], both[k]), k
    words = (b + 4) & ~3
    for run in (both, flagged):
        status = run["scratch"][run["scratch"].numel() - words:][:b + 1]
        assert not bool(status.any()), status.tolist()          # every role completed
    assert torch.equal(_without_arrival_slots(flagged["scratch"], b, nf, cap), _without_arrival_slots(both["scratch"], b, nf, cap))
    assert bool(_records(both["scratch"], b, nf, cap).any())
    assert bool(torch.isfinite(both["grad_verts"]).all()) and float(both["grad_verts"].abs().max()) > 0
    assert torch.equal(flagged["grad_verts"], both["grad_verts"])
    assert bool((flagged["idx_p"] == SENTINEL).all()) and bool((flagged["sq_gt"] == float(SENTINEL)).all())
    d1, i1, d2, i2 = chamfer_nn(both["gt"], both["points"])
    assert torch.equal(both["idx_p"], i1) and torch.equal(both["sq_gt"], d1) and torch.equal(flagged["idx_g"], i2)


# ---- python: utils.batch_point_to_surface drops the direction exactly where nothing reads it --------------------------------
@pytest.fixture
def scan_calls(monkeypatch):
    """(sq_gt argument, flags) of every geom_surface_scan_f32 the package issues from here on."""
    seen, real = [], L.call

    def spy(name, *args, **kwargs):
        if name == "geom_surface_scan_f32":
            seen.append((args[5], args[25]))
        return real(name, *args, **kwargs)

    monkeypatch.setattr(L, "call", spy)
    return seen


def _near_cloud(s, n_gt):
    """A gt cloud ON the meshes (their own samples from another seed), so that the F-score's threshold separates something."""
    ops.manual_seed(5)
    return ops.draw_samples(s["verts"], s["faces"], n_gt, with_points=True)[3].contiguous()


@pytest.mark.parametrize("shape", [(8, 2048, 1000), (2, 300, 200)], ids=["fused", "separate"])
def test_batch_point_to_surface_against_the_node_with_both_directions(gpu, scan_calls, shape):
    s = _scene(*shape)
    info, draws = utils.adj_init(s["faces"]), (s["choices"], s["u"], s["v"])
    gt = _near_cloud(s, s["n_gt"])
    verts = s["verts"].clone().requires_grad_(True)
    loss = utils.batch_point_to_surface(verts, info, gt, num=s["num"], draws=draws)
    loss.backward()
    assert len(scan_calls) == 1 and scan_calls[0][0] is None and scan_calls[0][1] & ONE          # no sq_gt, one direction
    ref_verts = s["verts"].clone().requires_grad_(True)
    ref_loss, ref_sq_gt, ref_sq_pred = ops.SurfaceLoss.apply(ref_verts, s["faces"], gt, *draws, False, utils.LOSS_SCALE)
    ref_loss.backward()
    assert scan_calls[1][0] is not None and not scan_calls[1][1] & ONE and ref_sq_gt is not None
    assert torch.equal(loss.detach(), ref_loss.detach()) and torch.equal(verts.grad, ref_verts.grad)
    assert float(verts.grad.abs().max()) > 0
    # the node itself, told that nobody reads the gt points' side
    out = ops.SurfaceLoss.apply(s["verts"], s["faces"], gt, *draws, False, utils.LOSS_SCALE, None, None, None, None, None, False)
    assert out[1] is None and torch.equal(out[0], ref_loss.detach()) and torch.equal(out[2], ref_sq_pred)
    # f1=True: both directions, the F-score of the two-direction scan
    loss_f, f_score = utils.batch_point_to_surface(s["verts"], info, gt, num=s["num"], f1=True, draws=draws)
    assert scan_calls[-1][0] is not None and not scan_calls[-1][1] & ONE
    points = utils.batch_sample(s["verts"], s["faces"], draws=draws).contiguous()          # the node's own gather of these draws
    d1, _, d2, _ = chamfer_nn(gt, points)
    assert f_score == utils._f_score(d1, d2, s["num"]) and 0.0 <= f_score < 1.0
    print("F-score %s: %.6f" % (shape, f_score))
    assert f_score > 0 or shape[1] < 2048          # the larger clouds are dense enough for the threshold to admit some points
    assert torch.equal(loss_f, ref_loss.detach())
    # the inspection hook promises idx_gt / sq_gt
    ops.scan_capture = seen = {}
    try:
        utils.batch_point_to_surface(s["verts"], info, gt, num=s["num"], draws=draws)
    finally:
        ops.scan_capture = None
    assert scan_calls[-1][0] is not None and not scan_calls[-1][1] & ONE
    e1, i1, _, i2 = chamfer_nn(gt, seen["points"])
    assert torch.equal(seen["idx_gt"], i1) and torch.equal(seen["idx_pred"], i2) and torch.equal(seen["sq_gt"], e1)


def test_truncation_mode_keeps_both_directions(gpu, scan_calls):
    import geometrics_amd
    s = _scene(2, 300, 200)
    info = utils.adj_init(s["faces"])
    try:
        geometrics_amd.set_reference_quirks(True)
        loss = utils.batch_point_to_surface(s["verts"], info, s["gt"], num=s["num"], draws=(s["choices"], s["u"], s["v"]))
    finally:
        geometrics_amd.set_reference_quirks(False)
    assert bool(torch.isfinite(loss)) and scan_calls[-1][0] is not None and not scan_calls[-1][1] & ONE


def _adam_step(gpu, both_directions, monkeypatch):
    b, n_gt, num = 5, 500, 300
    s = _scene(b, n_gt, num)
    info = utils.adj_init(s["faces"])
    csr = layers.adjacency_csr(info["adj"])
    torch.manual_seed(41)
    stack = [layers.Batch_Image_ZERON_GCNGCN(i, o).to(gpu) for i, o in ((48, 192), (192, 192), (192, 192))]
    g = torch.Generator(device="cpu").manual_seed(43)
    x = torch.randn(b, csr.nv, 48, generator=g).to(gpu)
    opt = optim.FusedAdam([p for layer in stack for p in layer.parameters()], lr=1e-3)
    monkeypatch.setattr(ops, "nn_both_directions", both_directions)
    with layers.deferred_parameter_gradients(), opt.in_backward():
        pos = layers.zero_n_stack_positions(x, csr, stack, F.relu, s["verts"], 0.01)
        utils.batch_point_to_surface(pos, info, s["gt"], num=num, draws=(s["choices"], s["u"], s["v"])).backward()
        stepped = bool(opt._stepped_in_backward)
    torch.cuda.synchronize()
    return stepped, [p.detach().clone() for p in opt.params] + list(opt.exp_avg) + list(opt.exp_avg_sq)


def test_adam_step_through_the_loss_equals_the_step_with_both_directions(gpu, scan_calls, monkeypatch):
    stepped_both, want = _adam_step(gpu, True, monkeypatch)
    stepped_one, got = _adam_step(gpu, False, monkeypatch)
    assert stepped_both and stepped_one
    assert [bool(flags & ONE) for _, flags in scan_calls] == [False, True]
    assert float(want[6].abs().max()) > 0          # (the first moment of the first weight did move)
    for i, (a, c) in enumerate(zip(got, want)):
        assert torch.equal(a, c), "tensor %d of parameters + exp_avg + exp_avg_sq differs" % i

"""-m gpu: the driver step that bench.py times (`driver_step`) held to the driver's own expressions.

bench.py's `driver_step_times` does not time the composition an unmodified driver issues (GEOMetrics.py:110-174) but an EDITED
one: the cameras formed once, poolings that write into a wide buffer (`headroom=`, `fronts=`), `utils.concat_features` for
`torch.cat`, `utils.fan_out` handles (6, 6 and 2 per stage), ONE stacked surface-loss call with a per-mesh weight vector, three
`utils.stage_regularisers` nodes with the driver's weights folded in by hand, `utils.sum_losses`, deferred parameter gradients
and `optim.FusedAdam`.  Every piece has a pairwise test; this module holds the pieces PUT TOGETHER:

* `edited_step` restates the branches bench.py takes with `zero_edit=False`, `DRIVER_STEP_STACKED_LOSSES = True` and no loss
  stream: `predict()` (bench.py:944-984), `losses()` (bench.py:986-995), `zero()` / `step()` (bench.py:997-1011), on the
  constants of bench.py:930 (`stage_weights`) and bench.py:942 (`base_const`).  bench.py's closures cannot be imported: the
  restatement is the point of contact, and a change to those lines has to be made here as well.
* `plain_step` restates the `zero_edit=True` branches (bench.py:1017-1034), which are the driver's own lines
  GEOMetrics.py:110-161 with their clones and `torch.cat`, on the same operators.

Both run at the driver's shapes (482-vertex template with its two 33-entry rows, blocks 963 / 1155 / 1155, four maps per stage)
on 3 meshes (a partly filled row tile) and 16 (the reference's batch), with 700 sampled against 900 ground-truth points (no tile
multiple; the smallest size at which the stacked call, the finalize pass and the gather backward all run) and the SAME draws.
The two forward passes are the same arithmetic on the same bits, so the ReLU masks agree and the two backward passes are one
linear map applied in two fp32 summation orders: no comparison here crosses a ReLU kink, which is what makes a whole-step
comparison against float64 loose or flaky (docstring of test_the_fused_block_against_float64_and_against_the_separate_operators).
Float64 is used where it is cheap and tight: the loss head with its hand-folded weights."""
import copy
import functools
import types

import numpy as np
import pytest
import torch

from helpers import fp64_surface_gradient, log_margin
from test_ops_parity_gpu import ROW_FLOOR_ULPS, ROW_RTOL_SURFACE
from geometrics_amd import backward_pass, deform, layers, meshgen, models, optim, utils
from oracle import ref_ops

pytestmark = pytest.mark.gpu

NUM, N_GT, HID = 700, 900, 192
MAPS = ((64, 56), (128, 28), (256, 14), (512, 7))
SEAMS = ("p1", "p2", "p3", "f1", "f2")


@functools.lru_cache(maxsize=None)
def _setup(gpu, batch):
    """What the compositions share, built once per batch size and never written: mesh, adjacency, ground truth, draws, cameras,
    pristine blocks and maps (every composition gets `copy.deepcopy`s / clones of them)."""
    V, Fc = meshgen.uv_sphere()
    nv = V.shape[0]
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    s = types.SimpleNamespace(batch=batch, nv=nv, V=V, Fc=Fc)
    s.info = utils.adj_init(to(Fc))
    s.csr = layers.adjacency_csr(s.info["adj"])
    assert nv == 482 and s.csr.ell_w == 8 and s.csr.over is not None      # the width-8 table plus the poles' tail
    s.initial = to(V)                                                     # 2-D, as the driver's load_initial returns it
    s.base_const = s.initial.unsqueeze(0).expand(batch, nv, 3).contiguous()               # bench.py:942
    s.gt_np = meshgen.gt_cloud(batch, N_GT, first=700)
    s.gt = to(s.gt_np)
    template = np.zeros((batch,) + V.shape, np.float32) + V
    s.draws_np = [meshgen.sampling_draws(template, Fc, NUM, first=10 * k) for k in range(3)]
    s.draws = [tuple(to(a) for a in d) for d in s.draws_np]
    s.all_draws = tuple(torch.cat([d[k] for d in s.draws]) for k in range(3))
    s.img_info = torch.tensor([[30.0 + 10 * i, 25.0, 1.1] for i in range(batch)], device=gpu)
    s.stage_weights = torch.tensor([3 * .2] * batch + [3 * .2] * batch + [3 * 2.0] * batch, dtype=torch.float32,
                                   device=gpu)                                            # bench.py:930
    torch.manual_seed(3041)
    s.blocks = [models.BatchMeshDeformationBlock(c, nv).to(gpu).train() for c in (963, 1155, 1155)]
    with torch.no_grad():
        for blk in s.blocks:
            for i in range(1, 14):
                getattr(blk, "bn%d" % i).weight.uniform_(0.5, 1.5)
                getattr(blk, "bn%d" % i).bias.uniform_(-0.3, 0.3)
    s.maps = [[torch.randn(batch, c, d, d, device=gpu) for c, d in MAPS] for _ in range(3)]
    return s


def _copies(s):
    return copy.deepcopy(s.blocks), [[m.clone().requires_grad_(True) for m in group] for group in s.maps]


def _zero(blocks, maps, opt=None):
    if opt is not None:
        opt.zero_grad()
    for blk in blocks:
        for p in blk.parameters():
            p.grad = None
    for group in maps:
        for m in group:
            m.grad = None


def _served(s, block, features, pooled):
    """One call of a block, on the fused training launches (`deform.enabled` at its default)."""
    assert deform.enabled and deform.serves(block, features, pooled, s.csr)
    return block(features, pooled, s.info["adj"])


def edited_head(s, p1, p2, p3):
    """bench.py:971-977 and 986-995 on the handles `utils.fan_out` returned: p1, p2 (six each; [3] the surface loss's, [4] the
    stage's regulariser as `cur`, [5] the next stage's as `prev`), p3 (two: surface loss, regulariser)."""
    s3 = utils.batch_point_to_surface(torch.cat((p1[3], p2[3], p3[0])), s.info, torch.cat((s.gt, s.gt, s.gt)), num=NUM,
                                      weight=s.stage_weights, draws=s.all_draws)
    return utils.sum_losses(
        s3,
        utils.stage_regularisers(s.initial, p1[4], s.info, lap_weight=.2 * .3 * 1500, edge_weight=300),
        utils.stage_regularisers(p1[5], p2[4], s.info, lap_weight=.2 * 1500, move_weight=.2 * 100, edge_weight=300),
        utils.stage_regularisers(p2[5], p3[1], s.info, lap_weight=.2 * 1500, move_weight=.2 * 100, edge_weight=300))


def edited_step(s, blocks, maps, opt=None):
    """bench.py's edited driver step (see the module docstring for the lines); opt: the step's `optim.FusedAdam`, stepped
    behind the backward pass as bench.py:1010 does.  Returns the loss and the seam tensors, their gradients retained."""
    _zero(blocks, maps, opt)
    seams = {}

    def seam(name, t):
        t.retain_grad()
        seams[name] = t
        return t
    with layers.deferred_parameter_gradients():
        base = s.base_const
        cam = utils.batch_camera_info(s.img_info)
        f = utils.batched_pooling(maps[0], base, cam, headroom=3, fronts=(base,))
        f, p1 = _served(s, blocks[0], base, f)
        seam("f1", f)
        p1 = utils.fan_out(seam("p1", base + p1), 6)
        f = utils.concat_features(f, utils.batched_pooling(maps[1], p1[0], cam, headroom=3 + HID, fronts=(p1[1], f)))
        f, p2 = _served(s, blocks[1], p1[1], f)
        seam("f2", f)
        p2 = utils.fan_out(seam("p2", p2 + p1[2]), 6)
        f = utils.concat_features(f, utils.batched_pooling(maps[2], p2[0], cam, headroom=3 + HID, fronts=(p2[1], f)))
        _, p3 = _served(s, blocks[2], p2[1], f)
        p3 = utils.fan_out(seam("p3", p3 + p2[2]), 2)
        loss = edited_head(s, p1, p2, p3)
        loss.backward()
    if opt is not None:
        opt.step()
    return types.SimpleNamespace(loss=loss.detach(), seams=seams)


def plain_step(s, blocks, maps, reverse_head=False):
    """GEOMetrics.py:110-161 as bench.py's zero-edit step issues it (bench.py:945-970 with zero_edit, 1017-1034): the cameras in
    front of every pooling, the clones, `torch.cat`, one surface loss per stage (the third with f1=True), the driver's own
    regulariser expressions and weights -- with replayed draws.  reverse_head: the same terms built in the opposite order
    (stage 3 first, Laplacian before edge before surface): the same maths on the same operators, only autograd's
    accumulation order at the positions differs -- the noise floor of a comparison between two fp32 orders."""
    _zero(blocks, maps)
    adj_info, initial_positions, img_info, gt_samples = s.info, s.initial, s.img_info, s.gt
    seams = {}

    def seam(name, t):
        t.retain_grad()
        seams[name] = t
        return t
    initial_positions_batch = initial_positions.unsqueeze(0).expand(s.batch, s.nv, 3)
    vertex_features = utils.batched_pooling(maps[0], initial_positions_batch, img_info.clone())
    vertex_features, vertex_positions_1 = _served(s, blocks[0], initial_positions_batch, vertex_features)
    seam("f1", vertex_features)
    p1 = seam("p1", initial_positions_batch + vertex_positions_1)
    vertex_features = torch.cat((vertex_features, utils.batched_pooling(maps[1], p1.clone(), img_info.clone())), dim=-1)
    vertex_features, vertex_positions_2 = _served(s, blocks[1], p1.clone(), vertex_features)
    seam("f2", vertex_features)
    p2 = seam("p2", vertex_positions_2 + p1)
    vertex_features = torch.cat((vertex_features, utils.batched_pooling(maps[2], p2.clone(), img_info.clone())), dim=-1)
    _, vertex_positions_3 = _served(s, blocks[2], p2.clone(), vertex_features)
    p3 = seam("p3", vertex_positions_3 + p2)

    p2s, edge, lap = utils.batch_point_to_surface, utils.batch_calc_edge, utils.batch_get_lap_info
    lap_term = lambda a, b: torch.mean(torch.sum((lap(a, adj_info) - lap(b, adj_info)) ** 2, 2)) * 1500
    move_term = lambda a, b: torch.mean(torch.sum((a - b) ** 2, 2)) * 100
    if not reverse_head:
        s1 = p2s(p1.clone(), adj_info, gt_samples, num=NUM, draws=s.draws[0])
        s2 = p2s(p2.clone(), adj_info, gt_samples, num=NUM, draws=s.draws[1])
        s3, f1 = p2s(p3.clone(), adj_info, gt_samples, num=NUM, f1=True, draws=s.draws[2])
        surface_loss = s1 * .2 + s2 * .2 + s3 * 2
        edge_loss = edge(p1.clone(), adj_info) * 300
        edge_loss += edge(p2.clone(), adj_info) * 300
        edge_loss += edge(p3.clone(), adj_info) * 300
        lap_loss_1 = lap_term(initial_positions, p1)
        lap_loss_2 = lap_term(p1, p2)
        lap_loss_2 += move_term(p1, p2)
        lap_loss_3 = lap_term(p2, p3)
        lap_loss_3 += move_term(p2, p3)
        lap_loss = .2 * (lap_loss_1 * .3 + lap_loss_2 + lap_loss_3)
        loss = edge_loss + surface_loss + lap_loss
    else:
        lap_loss_3 = lap_term(p2, p3)
        lap_loss_3 += move_term(p2, p3)
        lap_loss_2 = lap_term(p1, p2)
        lap_loss_2 += move_term(p1, p2)
        lap_loss_1 = lap_term(initial_positions, p1)
        lap_loss = .2 * (lap_loss_3 + lap_loss_2 + lap_loss_1 * .3)
        edge_loss = edge(p3.clone(), adj_info) * 300
        edge_loss += edge(p2.clone(), adj_info) * 300
        edge_loss += edge(p1.clone(), adj_info) * 300
        s3, f1 = p2s(p3.clone(), adj_info, gt_samples, num=NUM, f1=True, draws=s.draws[2])
        s2 = p2s(p2.clone(), adj_info, gt_samples, num=NUM, draws=s.draws[1])
        s1 = p2s(p1.clone(), adj_info, gt_samples, num=NUM, draws=s.draws[0])
        surface_loss = s3 * 2 + s2 * .2 + s1 * .2
        loss = lap_loss + edge_loss + surface_loss
    assert 0.0 <= f1 <= 1.0
    loss.backward()
    return types.SimpleNamespace(loss=loss.detach(), seams=seams)


def _named_gradients(blocks, maps):
    """{name: gradient or None} of every parameter and of the 12 maps."""
    out = {"block%d.%s" % (k, n): p.grad for k, blk in enumerate(blocks) for n, p in blk.named_parameters()}
    out.update({"maps%d[%d]" % (k, i): m.grad for k, group in enumerate(maps) for i, m in enumerate(group)})
    return out


def _running(blocks):
    return {"block%d.bn%d.%s" % (k, i, name): getattr(getattr(blk, "bn%d" % i), name)
            for k, blk in enumerate(blocks) for i in range(1, 14) for name in ("running_mean", "running_var")}


def _maxrel(got, want):
    """max |got - want| over max |want|."""
    got, want = got.detach().double(), want.detach().double()
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-30)


@pytest.mark.parametrize("batch", [3, 16])
def test_the_edited_step_against_the_drivers_expressions_over_two_iterations(gpu, batch):
    """`edited_step` against `plain_step`, tensor by tensor, twice.  The second iteration is the one in which the caching
    allocator hands back the addresses of the first one's wide buffers: the `ops._headroom` registry (keyed by storage address,
    `placed` entries of (data_ptr, _version, width)) and the in-place column slices of the blocks' input gradient meet stale
    state there.  Between the iterations the plain route's blocks are loaded with the edited route's (stepped) parameters and
    running statistics, so both start from the same bits again.

    1. forward, BIT FOR BIT: the three stages' positions, the two feature tensors handed from block to block, and the 39
       BatchNorm layers' moved running_mean / running_var;
    2. the loss at 1e-5 (the project's loss bar);
    3. the total gradient at p3 -- only the loss head -- at 1e-5 of its max-norm (the regularisers' bar; the stacked loss's is
       2e-6), at p2, p1 and the two feature tensors at 1e-4;
    4. the gradient of every parameter and of all 12 maps at 1e-4 of its max-norm, the suite's bar for a gradient computed in
       another fp32 summation order (module docstring of test_ops_parity_gpu.py); the six bn14 tensors None in both.  Beside
       every tensor's figure the run logs (helpers.log_margin, $GEOM_MARGIN_LOG) its NOISE FLOOR: the distance between
       `plain_step` and `plain_step(reverse_head=True)`, two orders of the plain composition alone.  A tensor beyond 1e-4
       while 1-3 hold is held to four times ITS floor (the edited composition regroups a sum in four places: two six-way
       fan-outs, the regularisers' lap(prev - cur), the stacked loss); beyond that it is a bug.  No bar comes from the edited
       composition's own output;
    5. (first iteration) the optimiser applied what the pass produced: `torch.optim.Adam` on a copy of the parameters as they
       were, fed clones of the edited route's gradients, agrees with the stepped parameters at 5e-6 of scale (the bar of
       test_fused_adam_many_tensors_and_graph_replay); the step count advanced by exactly one; no job of the pass is pending.

    Measured on an MI355X: see LAB_NOTES.md section 19."""
    s = _setup(gpu, batch)
    (e_blocks, e_maps), (p_blocks, p_maps), (r_blocks, r_maps) = _copies(s), _copies(s), _copies(s)
    params = [p for blk in e_blocks for p in blk.parameters()]
    names = ["block%d.%s" % (k, n) for k, blk in enumerate(e_blocks) for n, _ in blk.named_parameters()]
    assert len(params) == len(names) == 3 * 56
    opt = optim.FusedAdam(params, lr=1e-4)
    for it in range(2):
        tag = "driver step routes, batch %d, iteration %d: " % (batch, it)
        before = [p.detach().clone() for p in params]
        steps_before = opt.step_count
        e = edited_step(s, e_blocks, e_maps, opt)
        assert backward_pass.pending() == 0
        p = plain_step(s, p_blocks, p_maps)
        r = plain_step(s, r_blocks, r_maps, reverse_head=True)
        # 1. forward
        for name in SEAMS:
            assert torch.equal(e.seams[name], p.seams[name]), tag + "seam %s is not bit-equal" % name
            assert torch.equal(r.seams[name], p.seams[name]), tag + "seam %s of the reversed plain step" % name
        e_run, p_run = _running(e_blocks), _running(p_blocks)
        assert len(e_run) == 2 * 39
        for name in e_run:
            assert torch.equal(e_run[name], p_run[name]), tag + name
        # 2. loss
        e_loss, p_loss = float(e.loss), float(p.loss)
        ok = log_margin(tag + "loss", abs(e_loss - p_loss) / abs(p_loss), 1e-5)
        log_margin(tag + "loss [floor]", abs(float(r.loss) - p_loss) / abs(p_loss), 1e-5)
        assert ok, tag + "loss %r against %r" % (e_loss, p_loss)
        # 3. seam gradients
        for name in SEAMS:
            bar = 1e-5 if name == "p3" else 1e-4
            err = _maxrel(e.seams[name].grad, p.seams[name].grad)
            ok = log_margin(tag + "d loss / d %s" % name, err, bar)
            log_margin(tag + "d loss / d %s [floor]" % name, _maxrel(r.seams[name].grad, p.seams[name].grad), bar)
            assert ok, tag + "gradient at seam %s: %.3g of its scale (bar %g)" % (name, err, bar)
        # 4. every parameter and map gradient
        e_grad, p_grad = _named_gradients(e_blocks, e_maps), _named_gradients(p_blocks, p_maps)
        r_grad = _named_gradients(r_blocks, r_maps)
        unused = sorted(n for n, g in p_grad.items() if g is None)
        assert len(unused) == 6 and all(".bn14." in n for n in unused)
        assert sorted(n for n, g in e_grad.items() if g is None) == unused
        beyond = []
        for name, want in p_grad.items():
            if want is None:
                continue
            err, floor = _maxrel(e_grad[name], want), _maxrel(r_grad[name], want)
            ok = log_margin(tag + "grad " + name, err, 1e-4)
            log_margin(tag + "grad " + name + " [floor]", floor, 1e-4)
            if not ok and err <= 4 * floor:
                log_margin(tag + "grad " + name + " TOOK THE 4 x FLOOR BAR", err, 4 * floor)
            elif not ok:
                beyond.append("%s: %.3g of scale (bar 1e-4; 4 x its floor %.3g)" % (name, err, 4 * floor))
        assert not beyond, tag + "; ".join(beyond)
        # 5. the optimiser
        if it == 0:
            assert opt.step_count == steps_before + 1
            ref = [q.clone().requires_grad_(True) for q in before]
            for q, mine in zip(ref, params):
                q.grad = None if mine.grad is None else mine.grad.detach().clone()
            torch.optim.Adam(ref, lr=1e-4).step()
            for name, mine, q, was in zip(names, params, ref, before):
                if mine.grad is None:
                    assert torch.equal(mine.detach(), was), tag + name + " moved without a gradient"
                    continue
                err = _maxrel(mine, q)
                assert log_margin(tag + "Adam " + name, err, 5e-6), tag + "Adam %s: %.3g of scale" % (name, err)
        for mine, plain, rev in zip(e_blocks, p_blocks, r_blocks):
            plain.load_state_dict(mine.state_dict())
            rev.load_state_dict(mine.state_dict())


@pytest.mark.parametrize("batch", [3, 16])
def test_the_loss_head_with_its_folded_weights_against_float64(gpu, batch):
    """The head of the edited step alone -- the stacked surface call with its per-mesh weight vector, the three
    `stage_regularisers` nodes with the hand-folded weights (3 * .2, .2 * .3 * 1500, .2 * 100, ...), `sum_losses`, behind the
    fan-outs bench.py uses -- on the positions of one edited forward as leaves, against FLOAT64 of the driver's formula
    (GEOMetrics.py:134-161): the surface parts from helpers.fp64_surface_gradient per stage times .2 / .2 / 2, the regularisers
    from autograd over ref_ops.calc_edge / ref_ops.lap_info (the 2-D template as `prev` of stage 1).  Loss at 1e-5; every
    gradient element within w_s * (ROW_RTOL_SURFACE * mass + ROW_FLOOR_ULPS * floor) + 1e-5 * max |regulariser part|: the sum
    of the two bars those operators are already held to, no new number.  Independent of the plain composition."""
    s = _setup(gpu, batch)
    blocks, maps = _copies(s)
    e = edited_step(s, blocks, maps)
    pos = [e.seams[k].detach().cpu().numpy() for k in ("p1", "p2", "p3")]
    leaves = [torch.from_numpy(a).to(gpu).requires_grad_(True) for a in pos]
    loss = edited_head(s, utils.fan_out(leaves[0], 6), utils.fan_out(leaves[1], 6), utils.fan_out(leaves[2], 2))
    loss.backward()
    ws = (.2, .2, 2.0)
    surface = [fp64_surface_gradient(pos[k], s.Fc, s.gt_np, *s.draws_np[k], two_sided=False) for k in range(3)]
    faces_c = torch.from_numpy(s.Fc)
    adj_orig = ref_ops.calc_adj(faces_c).double()
    q = [torch.from_numpy(a).double().requires_grad_(True) for a in pos]
    li = lambda x: ref_ops.lap_info(x, adj_orig)
    edge_loss = sum(ref_ops.calc_edge(x, faces_c) * 300 for x in q)
    lap_loss_1 = torch.mean(torch.sum((li(torch.from_numpy(s.V).double()) - li(q[0])) ** 2, 2)) * 1500
    lap_loss_2 = torch.mean(torch.sum((li(q[0]) - li(q[1])) ** 2, 2)) * 1500 + torch.mean(torch.sum((q[0] - q[1]) ** 2, 2)) * 100
    lap_loss_3 = torch.mean(torch.sum((li(q[1]) - li(q[2])) ** 2, 2)) * 1500 + torch.mean(torch.sum((q[1] - q[2]) ** 2, 2)) * 100
    regularisers = edge_loss + .2 * (lap_loss_1 * .3 + lap_loss_2 + lap_loss_3)
    regularisers.backward()
    exact_loss = sum(w * part[0] for w, part in zip(ws, surface)) + float(regularisers.detach())
    tag = "driver step loss head, batch %d: " % batch
    got_loss = float(loss.detach())
    ok = log_margin(tag + "loss", abs(got_loss - exact_loss) / abs(exact_loss), 1e-5)
    assert ok, tag + "loss %r against float64 %r" % (got_loss, exact_loss)
    for k, (w, (_, grad, mass, floor)) in enumerate(zip(ws, surface)):
        reg = q[k].grad.numpy()
        bound = w * (ROW_RTOL_SURFACE * mass + ROW_FLOOR_ULPS * floor) + 1e-5 * np.abs(reg).max()
        err = np.abs(leaves[k].grad.cpu().numpy().astype(np.float64) - (w * grad + reg))
        worst = float((err / bound).max())
        ok = log_margin(tag + "d loss / d p%d, worst element over its bound" % (k + 1), worst, 1.0)
        assert ok, tag + "the gradient at p%d: worst element %.3g times its bound, max err %.3g of max %.3g" % (
            k + 1, worst, err.max(), np.abs(w * grad + reg).max())


def test_the_captured_step_replays_the_eager_step(gpu):
    """bench.py times HIP-graph replays of the step (bench.py:1051-1067).  At batch 16: three warm-up steps on a side stream, a
    snapshot of parameters, Adam moments, step state and BatchNorm buffers, ONE `edited_step` with its `opt.step()` captured
    (capture_error_mode="thread_local", as bench.py does) and replayed once; the snapshot restored IN PLACE (copy_ into the
    same tensors) and one eager `edited_step`.  Loss, seam positions, every parameter gradient, every stepped parameter,
    the moments and the running statistics: bit for bit.  The 12 map gradients at 1e-5 of scale: their per-texel lists fill in
    arrival order (as in test_block_input_assembled_in_place_equals_the_concatenations).  One process, one stream per phase."""
    s = _setup(gpu, 16)
    blocks, maps = _copies(s)
    params = [p for blk in blocks for p in blk.parameters()]
    opt = optim.FusedAdam(params, lr=1e-4)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            edited_step(s, blocks, maps, opt)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert opt.step_count == 3
    state = [p.data for p in params] + list(opt.exp_avg) + list(opt.exp_avg_sq) + [opt.state]
    state += [b for blk in blocks for b in blk.buffers() if b.dtype == torch.float32]
    snapshot = [t.clone() for t in state]

    def record(e):
        out = {"loss": e.loss.clone()}
        out.update({"seam " + k: t.detach().clone() for k, t in e.seams.items()})
        out.update({"d seam " + k: t.grad.clone() for k, t in e.seams.items()})
        out.update({"grad " + k: None if g is None else g.clone() for k, g in _named_gradients(blocks, maps).items()})
        out.update({"state %d" % i: t.clone() for i, t in enumerate(state)})
        return out
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        captured = edited_step(s, blocks, maps, opt)
    graph.replay()
    torch.cuda.synchronize()
    replayed = record(captured)
    assert opt.step_count == 4
    with torch.no_grad():
        for t, was in zip(state, snapshot):
            t.copy_(was)
    torch.cuda.synchronize()
    eager = record(edited_step(s, blocks, maps, opt))
    torch.cuda.synchronize()
    assert opt.step_count == 4 and backward_pass.pending() == 0
    assert replayed.keys() == eager.keys() and sum(k.startswith("grad maps") for k in eager) == 12
    for name, want in eager.items():
        got = replayed[name]
        if want is None or got is None:
            assert want is None and got is None and ".bn14." in name, name
        elif name.startswith("grad maps"):
            assert _maxrel(got, want) <= 1e-5, "%s: %.3g of scale" % (name, _maxrel(got, want))
        else:
            assert torch.equal(got, want), name
    moved = sum(not torch.equal(t, was) for t, was in zip(state[:len(params)], snapshot))
    assert moved == len(params) - 6          # the step really ran: everything but the bn14 tensors left the snapshot

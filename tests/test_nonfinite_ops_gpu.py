"""-m gpu: NaN and Inf through the pooling, the face sampler, FusedAdam and the ragged losses.

Every case has two halves.  REACH: the output elements that differ from the clean run (the same inputs without the planted value)
are exactly those the rule names; every other element is bit-identical to the clean run wherever the kernel's summation order
does not depend on the planted value (the pooling's map gradient is listed in arrival order: it meets its finite test's bound
instead).  KIND: inside the reach, helpers.nonfinite_close(kinds=True) against a float64 restatement wherever the reference's
expressions are defined; kinds=False only where the kind is indeterminate (Inf - Inf), said in the case.

The restatements and the planted faults they catch are tests/nonfinite_ops_helpers.py and tests/test_nonfinite_ops_host.py.  No
new tolerance: every finite comparison uses the bound of the finite test of the same kernel, named where it is used.

Measured margins of the finite parts (GEOM_MARGIN_LOG, one run on an MI355X; worst element as a share of its bound): Adam against
float64 torch.optim.Adam and against the written rule alike p 0.052, exp_avg 0.085, exp_avg_sq 0.62 (rtol 2e-5, atol 2e-6); the
pooling's map gradients 0.15 (8 eps of sum |P| |g|), its features beside a non-finite texel 0.16, its verts.grad there 0.083; the
ragged surface loss's verts.grad 0.42 one-sided / 0.33 two-sided (the finite test's own runs: 0.42 / 0.26); the ragged regularisers'
gradients 0.035.  Everything else in the file is an equality of bits, of masks or of kinds."""
import ctypes
import io

import numpy as np
import pytest
import torch

import draw_helpers as dh
import nonfinite_ops_helpers as nh
from geometrics_amd import _lib, meshgen, ops, optim, utils
from helpers import POOL_FLOOR_ULPS, POOL_NEAR, POOL_ROW_RTOL, fp64_surface_gradient, nonfinite_close
from oracle import ref_ops
from ragged_loss_helpers import batch_a
from ragged_reg_helpers import BATCHES, SCALAR_WEIGHTS, reference_value, union_chain
from test_draw_exact_gpu import _given, _restated_call
from test_nonfinite_gpu import _nan_exactly_when
from test_ops_parity_gpu import ROW_FLOOR_ULPS, ROW_RTOL_SURFACE
from test_pooling_vertex_gradient_gpu import POOL_P_ULPS, RAGGED_SHAPES, maps_and_gradient, ragged_inputs

pytestmark = pytest.mark.gpu

NAN, INF = nh.NAN, nh.INF


def _to(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _same_bits(a, b):
    """Two device tensors bit for bit; a NaN matches a NaN (its sign and payload are not pinned)."""
    if a.dtype != torch.float32:
        return a.shape == b.shape and bool(torch.equal(a, b))
    return nh.same_floats(a.detach().cpu().numpy(), b.detach().cpu().numpy())


def _differing(a, b):
    """Indices at which two float32 device vectors differ in the sense of _same_bits."""
    a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    both_nan = np.isnan(a) & np.isnan(b)
    return np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)) & ~both_nan).tolist()


# ---- B. the face sampler (csrc/draw_body.h) ----------------------------------------------------------------------------------
# The rule: a face whose fp32 area is NaN weighs nothing, exactly like a zero-area face, and every other face keeps its share
# (`run += area > 0 ? area : 0`).  No index is formed from a vertex position: the search runs over [0, nf - 1] whatever the table
# holds, the ragged route clamps every list entry (draw_ragged_face).  The visiting-order route (geom_surface_prepare_f32 with a
# gt_index): the order is a permutation built on the host from nan_to_num'ed centroids (tri_distance.kd_order), every entry of
# it is range-checked where it is followed (draw_samples_body, tri_prep_grouped_body), the corner table faces[order] holds
# vertex ids of the face list, the triangle records and the samples' index (nn_cull_emit) are written at loop positions.
SAMPLER_NUM = 1025               # a second sample chunk of one sample
SAMPLER_SEED, SAMPLER_OFFSET, SAMPLER_POSITION = 0x1234_5678_9ABC_DEF0 & (2 ** 63 - 1), 5 << 24, 3


def _sampler_mesh(level):
    V, faces = meshgen.icosphere(level)
    return meshgen.jittered_batch(V, 2), faces


def _sampler_uniforms(num):
    uniforms = np.random.default_rng(num).random((3, 2, num), dtype=np.float32)
    uniforms[0, :, :3] = [0.0, 1 - 2.0 ** -24, np.nextafter(np.float32(1), np.float32(0))]
    return uniforms


def _assert_finite_draws_off_the_vertex(faces, v, choices, *floats):
    assert not (faces[choices] == v).any(), "a face of the planted vertex was drawn"
    for t in floats:
        assert np.isfinite(t).all()


@pytest.mark.parametrize("where", ["low", "boundary", "last"])
@pytest.mark.parametrize("level", [2, 3])
def test_sampler_given_uniforms_with_a_nan_vertex(gpu, level, where):
    """geom_draw_samples_f32, B = 2, NaN in one vertex of mesh 0: choices, u and v of both meshes are the extended restatement's
    bit for bit, no chosen face touches the vertex, mesh 1 is bit-identical to the clean run."""
    verts, faces = _sampler_mesh(level)
    v = nh.sampler_plants(faces)[where]
    planted = verts.copy()
    planted[0] = nh.planted_vertex(verts[0], v, NAN)
    uniforms = _sampler_uniforms(SAMPLER_NUM)
    clean = _given(gpu, verts, faces, uniforms)
    got = _given(gpu, planted, faces, uniforms)
    for m in range(2):
        ref_c, ref_u, ref_v, _ = dh.draw(planted[m], faces, uniforms[0, m], uniforms[1, m], uniforms[2, m])
        assert np.array_equal(got[0][m], ref_c), "mesh %d: choices" % m
        assert nh.same_floats(got[1][m], ref_u) and nh.same_floats(got[2][m], ref_v)
    _assert_finite_draws_off_the_vertex(faces, v, got[0][0], got[1][0], got[2][0])
    for g, c in zip(got, clean):
        assert np.array_equal(g[1], c[1]), "the other mesh changed"
    assert not np.array_equal(got[0][0], clean[0][0])


def _rng_call(gpu, verts, faces, num=SAMPLER_NUM):
    state = ops.manual_seed(SAMPLER_SEED, gpu, mesh_offset=SAMPLER_OFFSET)
    try:
        state[1] = SAMPLER_POSITION
        got = ops.draw_samples(_to(verts, gpu), _to(faces, gpu), num, with_points=True)
        return [t.cpu().numpy() for t in got], ops._rng_state(gpu).cpu().tolist()
    finally:
        ops.manual_seed(0, gpu)


@pytest.mark.parametrize("value", ["nan", "+inf"])
@pytest.mark.parametrize("where", ["low", "boundary", "last"])
@pytest.mark.parametrize("level", [2, 3])
def test_sampler_stream_with_a_non_finite_vertex(gpu, level, where, value):
    """geom_draw_samples_rng_f32 (ops.draw_samples(with_points=True)), B = 2, num = 1025, the value in one vertex of mesh 0:
    choices, u, v and points are the restatement's bit for bit (a NaN point is NaN in both), mesh 1 is bit-identical to the clean
    run and the state reads [seed, position + 1, 0, first mesh].  NaN: no chosen face touches the vertex, everything drawn is
    finite.  +Inf (areas +Inf or NaN, face by face): every choice is in [0, nf) -- what is drawn is what the restatement gives,
    DESIGN.md states it."""
    verts, faces = _sampler_mesh(level)
    v = nh.sampler_plants(faces)[where]
    planted = verts.copy()
    planted[0] = nh.planted_vertex(verts[0], v, nh.VALUES[value])
    clean, _ = _rng_call(gpu, verts, faces)
    got, state = _rng_call(gpu, planted, faces)
    want = _restated_call(planted, faces, SAMPLER_SEED, SAMPLER_POSITION, SAMPLER_OFFSET, SAMPLER_NUM)
    assert state == [SAMPLER_SEED, SAMPLER_POSITION + 1, 0, SAMPLER_OFFSET]
    assert np.array_equal(got[0], want[0]), "choices"
    for k, name in ((1, "u"), (2, "v"), (3, "points")):
        assert nh.same_floats(got[k], want[k]), name
    assert got[0].min() >= 0 and got[0].max() < faces.shape[0]
    for g, c in zip(got, clean):
        assert np.array_equal(g[1], c[1]), "the other mesh changed"
    if value == "nan":
        _assert_finite_draws_off_the_vertex(faces, v, got[0][0], got[1][0], got[2][0], got[3][0])
    else:
        assert np.isfinite(got[1]).all() and np.isfinite(got[2]).all()


@pytest.mark.parametrize("value", ["nan", "+inf"])
@pytest.mark.parametrize("where", ["low", "boundary", "last"])
def test_sampler_visiting_order_route_with_a_non_finite_vertex(gpu, where, value):
    """ops.draw_samples(prepare_scan_for=, gt_index=) at the shape of test_visiting_order_route (level 3, B 6, num 1000, n_gt
    2750: the samples are generated in visiting order), the value in one vertex of mesh 1 -- a vertex of the first, of a middle
    and of the last face OF THE VISITING ORDER (the table is built over it).  The face's uniform comes from __logf there and
    cannot be restated; what can: the route ran, u and v are sqrt(u01(word y)) and u01(word z) of the restated stream bit for
    bit, the points are those of the chosen faces bit for bit, every choice is in [0, nf) and its position in the visiting order
    never decreases, the other five meshes are bit-identical to the clean call, the state reads [seed, position + 1, 0, first
    mesh].  NaN: no chosen face touches the vertex and everything drawn is finite -- and the faces behind the first NaN one are
    still drawn (the unconditional running sum lost them: with the vertex on the first face every sample went to the last)."""
    from geometrics_amd.tri_distance import face_order
    B, num, n_gt, mesh = 6, 1000, 2750, 1
    V, faces = meshgen.icosphere(3)
    nf = faces.shape[0]
    verts = meshgen.jittered_batch(V, B)
    df, gt = _to(faces, gpu), _to(meshgen.gt_cloud(B, n_gt), gpu)
    gi = ops.GtIndex(gt)
    order = face_order(_to(verts, gpu), df).long()             # (cached per face tensor: the clean and the planted call share it)
    order_np = order.cpu().numpy()
    assert np.array_equal(np.sort(order_np), np.arange(nf))
    rank = np.empty(nf, np.int64)
    rank[order_np] = np.arange(nf)
    v = nh.sampler_plants(faces[order_np])[where]
    planted = verts.copy()
    planted[mesh] = nh.planted_vertex(verts[mesh], v, nh.VALUES[value])

    def call(x):
        state = ops.manual_seed(SAMPLER_SEED, gpu, mesh_offset=SAMPLER_OFFSET)
        try:
            state[1] = SAMPLER_POSITION
            d = ops.draw_samples(_to(x, gpu), df, num, with_points=True, prepare_scan_for=n_gt, gt_index=gi)
            assert isinstance(d[4], ops.ScanPrep) and d[4].sample_index is not None, "the visiting-order generation did not run"
            return [t.cpu().numpy() for t in d[:4]], ops._rng_state(gpu).cpu().tolist()
        finally:
            ops.manual_seed(0, gpu)

    clean, _ = call(verts)
    got, state = call(planted)
    assert state == [SAMPLER_SEED, SAMPLER_POSITION + 1, 0, SAMPLER_OFFSET]
    choices, u, w, points = got
    assert choices.min() >= 0 and choices.max() < nf
    assert (np.diff(rank[choices], axis=1) >= 0).all()
    for m in range(B):
        _, r1, r2 = dh.stream_uniforms(SAMPLER_SEED, SAMPLER_POSITION, SAMPLER_OFFSET + m, num)
        assert nh.same_floats(u[m], np.sqrt(r1)) and nh.same_floats(w[m], r2), "mesh %d" % m
        assert nh.same_floats(points[m], dh.sampled_points(planted[m], faces, choices[m], u[m], w[m])), "mesh %d: points" % m
        if m != mesh:
            for g, c in zip(got, clean):
                assert np.array_equal(g[m], c[m]), "mesh %d changed" % m
    if value == "nan":
        _assert_finite_draws_off_the_vertex(faces, v, choices[mesh], u[mesh], w[mesh], points[mesh])
        touched = rank[nh.faces_of_vertex(faces, v)]
        if where != "last":
            behind = rank[choices[mesh]] > touched.min()
            assert len(set(choices[mesh][behind].tolist())) > 50, "the faces behind the first NaN face are not drawn"
    assert not np.array_equal(choices[mesh], clean[0][mesh])


@pytest.fixture(scope="module")
def ragged_a(gpu):
    from test_ragged_loss_gpu import OnDevice
    return OnDevice(batch_a(), gpu)


def _ragged_call(gpu, d, verts, num=SAMPLER_NUM):
    state = ops.manual_seed(SAMPLER_SEED, gpu, mesh_offset=SAMPLER_OFFSET).clone()
    state[1] = SAMPLER_POSITION
    choices = torch.full((d.b, num), -1, dtype=torch.int64, device=gpu)
    u, v, pts = torch.zeros(d.b, num, device=gpu), torch.zeros(d.b, num, device=gpu), torch.zeros(d.b, num, 3, device=gpu)
    _lib.call("geom_draw_samples_ragged_f32", d.b, verts.shape[0], verts, d.faces.shape[0], d.faces, d.face_list, d.face_off, num,
              None, state, choices, u, v, pts)
    ops.manual_seed(0, gpu)
    return [t.cpu().numpy() for t in (choices, u, v, pts)], state.cpu().tolist()


@pytest.mark.parametrize("value", ["nan", "+inf"])
@pytest.mark.parametrize("where", ["low", "boundary", "last"])
def test_ragged_sampler_with_a_non_finite_vertex(gpu, ragged_a, where, value):
    """geom_draw_samples_ragged_f32 on ragged_loss_helpers.batch_a(), the value in one vertex of the 1025-face mesh (two faces per
    thread): every mesh is the restatement of ITS faces on the union vertices, bit for bit, as union face ids; the other seven
    meshes are bit-identical to the clean run; the state advances once."""
    d, rb, mesh = ragged_a, ragged_a.rb, 6
    ids, faces_m = rb.faces_of(mesh)
    assert faces_m.shape[0] == 1025
    v = nh.sampler_plants(faces_m)[where]
    planted = nh.planted_vertex(rb.verts, v, nh.VALUES[value])
    clean, _ = _ragged_call(gpu, d, d.verts)
    got, state = _ragged_call(gpu, d, _to(planted, gpu))
    assert state == [SAMPLER_SEED, SAMPLER_POSITION + 1, 0, SAMPLER_OFFSET]
    assert got[0].min() >= 0 and got[0].max() < rb.faces.shape[0]
    for m in range(rb.b):
        ids_m, f_m = rb.faces_of(m)
        c, u, w, pts = dh.draw(planted, f_m, *dh.stream_uniforms(SAMPLER_SEED, SAMPLER_POSITION, SAMPLER_OFFSET + m, SAMPLER_NUM))
        assert np.array_equal(got[0][m], ids_m[c]), "mesh %d: choices" % m
        assert nh.same_floats(got[1][m], u) and nh.same_floats(got[2][m], w) and nh.same_floats(got[3][m], pts), "mesh %d" % m
        if m != mesh:
            for g, cl in zip(got, clean):
                assert np.array_equal(g[m], cl[m]), "mesh %d changed" % m
    if value == "nan":
        _assert_finite_draws_off_the_vertex(rb.faces, v, got[0][mesh], got[1][mesh], got[2][mesh], got[3][mesh])
    assert not np.array_equal(got[0][mesh], clean[0][mesh])


# ---- C. FusedAdam (csrc/adam.hip, adam_math.h, dense_gemm.hip reduce_body) -----------------------------------------------------
# No index or address depends on a gradient, a moment or a parameter VALUE on any route.  The three routes: the chunked launch
# (geom_adam_step_f32), the table launch (geom_adam_table_step_f32) and the update inside the end-of-pass reduction
# (geom_dense_reduce_adam_f32), which is driven here on the launch itself: the gradient of tensor i is the column sum of a
# three-row partial (the planted value sits in one of the rows: a column-sum job), the last tensor's the 192 x 192 weight gradient
# x^T g of a weight job; the launch finishes them and steps, and the other two routes are handed the finished gradients.  A
# column-sum job takes whole groups of four columns, so that route runs on REDUCE_SIZES.  (A planted value cannot be ONE element
# of a weight gradient: an element of g is a column of x^T g.)
ISSUE_SIZES = (1, 7, 1023, 1025, 192 * 192)
REDUCE_SIZES = (4, 8, 1024, 1028, 192 * 192)
ADAM_PLANTS = [("first", 4, 0), ("last", 4, -1), ("at_1024", 3, 1024), ("before_1024", 3, 1023), ("smallest", 0, 0)]


WEIGHT_ROWS, WEIGHT_W = 83, 192          # the reduction launch's weight job: grad_w [192, 192] = x^T g over 83 rows (test_dense_gpu.SHAPES)


def _adam_inputs(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(n, generator=g) for n in sizes]
    partials = [[torch.randn(3, n, generator=g) for n in sizes] for _ in range(3)]      # per step: the three rows a gradient sums
    x = torch.randn(WEIGHT_ROWS, WEIGHT_W, generator=g)
    gs = [torch.randn(WEIGHT_ROWS, WEIGHT_W, generator=g) for _ in range(3)]              # per step: the weight job's output gradient
    return params, partials, x, gs


class _Route:
    def __init__(self, name, params, gpu):
        self.name = name
        self.p = [t.clone().to(gpu).requires_grad_(True) for t in params]
        self.opt = optim.FusedAdam(self.p, lr=nh.ADAM_LR, betas=nh.ADAM_BETAS, eps=nh.ADAM_EPS, table=(name == "table"))

    def step(self, partials, grads, x=None, g=None):
        """One step on the gradients `grads` (chunked, table) or on what the reduction launch finishes them from (reduce): the
        three partial rows of every column-sum job and, for the LAST tensor, the weight job's split partial tiles of x^T g.
        Returns the gradients used."""
        opt = self.opt
        if self.name != "reduce":
            for p, gr in zip(self.p, grads):
                p.grad = gr.clone()
            opt.step()
            return grads
        from geometrics_amd import dense
        n = len(self.p) - 1
        outs = [torch.empty_like(p.detach()) for p in self.p]
        ws = dense.weight_workspace(WEIGHT_ROWS, WEIGHT_W, WEIGHT_W, x.device)
        dense.backward_weight_partials(x, g, ws)
        ints = lambda seq: (ctypes.c_int * len(seq))(*seq)
        pick = lambda seq: ([seq[-1]], list(seq[:-1]))
        (w_p, b_p), (w_m, b_m), (w_v, b_v) = pick([p.detach() for p in self.p]), pick(opt.exp_avg), pick(opt.exp_avg_sq)
        _lib.call("geom_dense_reduce_adam_f32", 1, ints([WEIGHT_ROWS]), ints([WEIGHT_W]), ints([WEIGHT_W]), [ws], [outs[-1]], w_p, w_m, w_v,
                  n, partials, ints([3] * n), ints([p.numel() for p in self.p[:-1]]), outs[:-1], b_p, b_m, b_v,
                  float(opt.lr), float(opt.betas[0]), float(opt.betas[1]), float(opt.eps), opt.state)
        opt._stepped = [True] * len(self.p)
        return outs

    def snapshot(self):
        torch.cuda.synchronize()
        return ([p.detach().clone() for p in self.p], [m.clone() for m in self.opt.exp_avg], [v.clone() for v in self.opt.exp_avg_sq],
                self.opt.state.clone())


def _adam_run(gpu, sizes, routes, plant):
    """Three steps on every route: {route: [snapshot after step 1, 2, 3]} and the gradients of every step (float32, host).
    plant = (tensor, element, value, "grad" | "param") or None: in the gradient of steps 1 and 2, or in the parameter."""
    params, partials, x, gs = _adam_inputs(sizes, 17)
    if "reduce" in routes:
        params.append(torch.randn(WEIGHT_W * WEIGHT_W, generator=torch.Generator().manual_seed(18)))
    if plant and plant[3] == "param":
        params[plant[0]][plant[1]] = plant[2]
    if plant and plant[3] == "grad":
        for step in (0, 1):
            partials[step][plant[0]][1, plant[1]] = plant[2]
    if plant and plant[3] == "column":        # one element of the weight job's output gradient: a whole column of x^T g
        for step in (0, 1):
            gs[step][40, plant[1]] = plant[2]
    partials = [[t.to(gpu) for t in step] for step in partials]
    x, gs = x.to(gpu), [t.to(gpu) for t in gs]
    out, used = {r: [] for r in routes}, []
    made = {r: _Route(r, params, gpu) for r in routes}
    for step in range(3):
        grads = None
        if "reduce" in made:
            grads = made["reduce"].step(partials[step], None, x, gs[step])
            out["reduce"].append(made["reduce"].snapshot())
        else:
            grads = [(t[0] + t[1]) + t[2] for t in partials[step]]
        for r in routes:
            if r != "reduce":
                made[r].step(None, grads)
                out[r].append(made[r].snapshot())
        used.append([g.cpu().numpy() for g in grads])
    return out, used, [t.numpy() for t in params], made


@pytest.fixture(scope="module")
def adam_clean(gpu):
    return {"issue": _adam_run(gpu, ISSUE_SIZES, ("chunked", "table"), None)[0],
            "reduce": _adam_run(gpu, REDUCE_SIZES, ("reduce", "chunked", "table"), None)[0]}


def _adam_check(gpu, adam_clean, sizeset, plant):
    sizes, routes = (ISSUE_SIZES, ("chunked", "table")) if sizeset == "issue" else (REDUCE_SIZES, ("reduce", "chunked", "table"))
    tensor, element, value, kind = plant
    base_sizes = sizes
    if sizeset == "reduce":
        sizes = sizes + (WEIGHT_W * WEIGHT_W,)
    element = element % sizes[tensor]
    got, used, params, made = _adam_run(gpu, base_sizes, routes, (tensor, element, value, kind))
    # the planted element; a planted column of the weight job's output gradient is column `element` of x^T g: 192 elements
    planted = [element + WEIGHT_W * i for i in range(WEIGHT_W)] if kind == "column" else [element]
    if kind != "param":
        for step in (0, 1):           # the finished gradient is not finite in exactly those elements
            bad = [np.flatnonzero(~np.isfinite(g)).tolist() for g in used[step]]
            assert bad == [planted if i == tensor else [] for i in range(len(sizes))]
            if kind == "grad":
                assert np.isnan(used[step][tensor][element]) if np.isnan(value) else used[step][tensor][element] == value
        assert all(np.isfinite(g).all() for g in used[2])
    ref, rule = nh.adam_torch64(params, used), nh.adam_rule64(params, used)
    first = routes[0]
    for step in range(3):
        for r in routes:
            snap, base = got[r][step], adam_clean[sizeset][r][step]
            # the step state and the re-armed arrival counters are the clean run's
            assert _same_bits(snap[3], base[3]) and float(snap[3][0]) == step + 1
            assert int(snap[3].view(torch.int32)[3:].abs().sum()) == 0
            for k, name in enumerate(("p", "exp_avg", "exp_avg_sq")):
                for i in range(len(sizes)):
                    what = "%s %s[%d] after step %d" % (r, name, i, step + 1)
                    # reach: the planted element alone (p alone for a planted parameter); every other element is the clean run's
                    differs = _differing(snap[k][i], base[k][i])
                    reach = planted if i == tensor and (kind != "param" or name == "p") else []
                    assert differs == reach, what + ": differs from the clean run at %s" % differs[:8]
                    # the routes agree bit for bit, NaN positions included
                    assert _same_bits(snap[k][i], got[first][step][k][i]), what + " against " + first
                    # kind: float64.  m behind an infinite gradient from the second step on: torch forms Inf - Inf in its lerp
                    # (NaN), the written rule keeps the Inf -- the kind is indeterminate against torch (mask only) and pinned
                    # against the rule
                    lerp = name == "exp_avg" and kind != "param" and np.isinf(value) and step > 0
                    want = ref[step][k][i]
                    nonfinite_close(snap[k][i], want, nh.adam_mass(want), nh.ADAM_RTOL, what, kinds=not lerp)
                    want = rule[step][k][i]
                    nonfinite_close(snap[k][i], want, nh.adam_mass(want), nh.ADAM_RTOL, what + " (the written rule)", kinds=True)
    return made


@pytest.mark.parametrize("value", ["nan", "+inf", "-inf"])
@pytest.mark.parametrize("where,tensor,element", ADAM_PLANTS, ids=[p[0] for p in ADAM_PLANTS])
@pytest.mark.parametrize("sizeset", ["issue", "reduce"])
def test_adam_with_a_non_finite_gradient_element(gpu, adam_clean, sizeset, where, tensor, element, value):
    """One gradient element NaN / +Inf / -Inf on steps 1 and 2, a clean third step: the first and the last element of the 192 x 192
    tensor, elements 1023 and 1024 of the 1025- (1028-) element tensor -- either side of a workgroup's span of 1024 (256 in the
    reduction launch) --, the tensor of one (four) elements.  After every step, on every route: p, exp_avg and exp_avg_sq against
    torch.optim.Adam in float64 (nonfinite_close, the finite bound of test_table_route_tracks_torch_adam); every element but the
    planted one bit-identical to the clean run of the same route; the routes bit-identical to each other; step state and arrival
    counters those of the clean run.  'issue': sizes 1, 7, 1023, 1025, 192 * 192 on the chunked and the table launch.  'reduce': sizes 4, 8, 1024, 1028, 192 * 192 on all three."""
    _adam_check(gpu, adam_clean, sizeset, (tensor, element, nh.VALUES[value], "grad"))


@pytest.mark.parametrize("value", ["nan", "+inf", "-inf"])
@pytest.mark.parametrize("column", [0, 191])
def test_adam_with_a_non_finite_weight_gradient_column(gpu, adam_clean, column, value):
    """The reduction launch's WEIGHT job: grad_w = x^T g out of the split partial tiles of a [83, 192] x [83, 192] product, one
    element of g not finite -- column `column` of the 192 x 192 gradient (NaN, or +-Inf by the sign of x: what the float64
    product of the finished gradient's operands gives is what the kernel finished, asserted through the reach).  Those 192
    elements of p and both moments follow float64, every other element of every tensor is the clean run's, the chunked and the
    table launch on the finished gradient agree with the reduction launch bit for bit."""
    _adam_check(gpu, adam_clean, "reduce", (len(REDUCE_SIZES), column, nh.VALUES[value], "column"))


@pytest.mark.parametrize("value", ["nan", "+inf"])
@pytest.mark.parametrize("sizeset", ["issue", "reduce"])
def test_adam_with_a_non_finite_parameter(gpu, adam_clean, sizeset, value):
    """The value in a PARAMETER (element 3 of the second tensor), clean gradients: p stays non-finite there, both moments and
    every other element are the clean run's, on every route."""
    _adam_check(gpu, adam_clean, sizeset, (1, 3, nh.VALUES[value], "param"))


def test_adam_checkpoint_carries_non_finite_moments(gpu, adam_clean):
    """state_dict() through torch.save / torch.load into load_state_dict() of a fresh optimiser: NaN and Inf moments unchanged, bit
    for bit, with the step state."""
    made = _adam_check(gpu, adam_clean, "issue", (3, 1024, INF, "grad"))
    opt = made["table"].opt
    assert bool(torch.isinf(opt.exp_avg[3][1024])) and bool(torch.isinf(opt.exp_avg_sq[3][1024]))
    made_nan = _adam_check(gpu, adam_clean, "issue", (4, 0, NAN, "grad"))
    for src in (opt, made_nan["chunked"].opt):
        buf = io.BytesIO()
        torch.save(src.state_dict(), buf)
        buf.seek(0)
        sd = torch.load(buf, weights_only=False)
        fresh = optim.FusedAdam([p.detach().clone().requires_grad_(True) for p in src.params], lr=nh.ADAM_LR)
        fresh.load_state_dict(sd)
        for a, b in zip(fresh.exp_avg + fresh.exp_avg_sq, src.exp_avg + src.exp_avg_sq):
            assert _same_bits(a, b)
        assert not all(bool(torch.isfinite(m).all()) for m in fresh.exp_avg)
        assert _same_bits(fresh.state[:3], src.state[:3]) and fresh.step_count == 3


# ---- A. pooling and camera (csrc/pooling.hip) --------------------------------------------------------------------------------
# The index path: project() forms xs, ys from the vertex and the camera; texel() is the only place they become indices, through
# fminf(fmaxf(r, 0), hi) -- 0 for a NaN, a bound for +-Inf --, so every texel index lies in [0, dim * dim) and the pair a quad_of
# read starts at (yb <= dim - 2) lies inside the row.  pool_bin_body counts and lists through those same indices and through
# vertex ids of its own loop; a map VALUE or a gradient VALUE is never an index.  The rules:
#   * a vertex whose projection is NaN -- a NaN or, through Inf / Inf in the perspective divide, an infinite coordinate; every
#     vertex of a mesh whose camera is NaN -- stands at texel 0 with four zero weights: its pooled row is 0 * that texel, its
#     verts.grad row is exactly zero (the clamp is a select), it adds nothing to a map gradient;
#   * a non-finite texel reaches the rows that READ it, also with weight zero (the forward forms 0 * NaN, as the reference);
#     the texel beside it in a paired read is never selected;
#   * a non-finite output-gradient element reaches the texels its vertex holds with NON-ZERO weight (corners() drops the others:
#     a sparse sum like the aggregation's) and that vertex's verts.grad row.

EPS = float(np.finfo(np.float32).eps)
MAP_RTOL = 8 * EPS               # test_pooling_map_gradient_per_element_at_the_training_shape's: 8 eps * sum |P| |g|
POOL_FORMS = [(0, True), (7, True), (0, False), (7, False)]          # (headroom, the maps want a gradient)
POOL_PLANT_MAP = {"four_maps": 1, "two_maps": 1}                     # the 130 x 9 x 9 and the 64 x 13 x 13 map


def _pool_run(gpu, verts, cams, maps, grad_out, headroom, maps_want_grad):
    """(features, verts.grad, [map gradients]) of utils.batched_pooling with the gradient handed in pitched when headroom > 0."""
    v = verts.to(gpu).requires_grad_(True)
    m = [t.to(gpu).requires_grad_(maps_want_grad) for t in maps]
    feats = utils.batched_pooling(m, v, cams, headroom=headroom)
    wide = torch.zeros(grad_out.shape[0], grad_out.shape[1], headroom + grad_out.shape[2], device=gpu)
    wide[..., headroom:] = grad_out.to(gpu)
    got = torch.autograd.grad(feats, [v] + (m if maps_want_grad else []), wide[..., headroom:])
    torch.cuda.synchronize()
    return feats.detach().clone(), got[0], list(got[1:])


class _PoolCase:
    """One of RAGGED_SHAPES on ragged_inputs(): the inputs, the fp32 cameras, the clean run of every launch form, the kernel's own
    P per map (identity maps pooled: the finite map-gradient test's reference) and the float64 texel tables of the rule."""

    def __init__(self, gpu, shape):
        self.chans, self.dims = RAGGED_SHAPES[shape]
        self.verts, self.img_info = ragged_inputs()
        self.maps, self.grad_out = maps_and_gradient(32, self.verts, self.chans, self.dims)
        self.cams = utils.batch_camera_info(self.img_info.to(gpu))
        self.host_cams = tuple(t.cpu() for t in self.cams)
        self.clean = {form: _pool_run(gpu, self.verts, self.cams, self.maps, self.grad_out, *form) for form in POOL_FORMS}
        self.P = [self.kernel_P(gpu, self.verts, self.cams, d) for d in self.dims]
        self.tables = [nh.pool_weights64(self.verts, *self.host_cams, d) for d in self.dims]
        zeros = [torch.zeros(2, 1, d, d) for d in self.dims]
        self.keep = ref_ops.pool_vertex_gradient(zeros, self.verts, *self.host_cams, torch.zeros(2, 101, len(self.dims)))[3] >= POOL_NEAR
        self.cols = np.concatenate(([0], np.cumsum(self.chans)))

    @staticmethod
    def kernel_P(gpu, verts, cams, d):
        b = verts.shape[0]
        eye = torch.eye(d * d, device=gpu).view(1, d * d, d, d).expand(b, -1, -1, -1).contiguous()
        return utils.batched_pooling([eye], verts.to(gpu), cams).double().cpu()          # [b, nv, d * d]

    def map_gradient_close(self, got, P, grad_out, what):
        """Every map gradient against P^T g in float64 at the finite test's bound."""
        g = grad_out.double()
        for l, (c, d, gm) in enumerate(zip(self.chans, self.dims, got)):
            gl = g[..., self.cols[l]:self.cols[l + 1]]
            ref = torch.einsum("bvt,bvc->bct", P[l], gl).view(2, c, d, d)
            mass = torch.einsum("bvt,bvc->bct", P[l].abs(), gl.abs()).view(2, c, d, d)
            nonfinite_close(gm, ref, mass, MAP_RTOL, "%s, map %d x %d" % (what, d, d))


@pytest.fixture(scope="module")
def pool_cases(gpu):
    return {shape: _PoolCase(gpu, shape) for shape in RAGGED_SHAPES}


def _rows_differing(got, clean):
    g, c = got.detach().cpu().numpy(), clean.detach().cpu().numpy()
    same = (g.view(np.uint32) == c.view(np.uint32)) | (np.isnan(g) & np.isnan(c))
    return {(int(b), int(v)) for b, v in np.argwhere(~same.all(-1))}


POOL_VERTS = [(0, 17), (1, 100)]         # an ordinary vertex of mesh 0; the last vertex of mesh 1 (the ragged tile of 37)


@pytest.mark.parametrize("value", ["nan", "+inf", "-inf"])
@pytest.mark.parametrize("shape", sorted(RAGGED_SHAPES))
def test_pooling_with_a_non_finite_vertex_coordinate(gpu, pool_cases, shape, value):
    """NaN, +Inf, -Inf in one coordinate of a vertex.  An infinite coordinate makes X, Y, Z infinite and the perspective divide
    Inf / Inf: the float64 projection is NaN as well (asserted; ref_ops.pool_features would convert a NaN to an index there), so
    all three follow the NaN rule.  The vertex's pooled row is exactly zero (finite maps) and what 0 * texel 0 gives where
    that texel is not finite, its verts.grad row exactly zero; every other row of both is bit-identical to the clean run; the map
    gradients meet the finite test's bound against the gradient of the batch WITHOUT that vertex (the clean run's P, its row
    zeroed).  Both vertices, headroom 0 and 7, both backward launch forms."""
    case = pool_cases[shape]
    for mesh, v in POOL_VERTS:
        verts = case.verts.clone()
        verts[mesh, v, 1] = nh.VALUES[value]
        _, _, _, xs, ys = ref_ops._pool_project(verts.double(), *(t.double() for t in case.host_cams))
        assert bool(torch.isnan(xs[mesh, v])) and bool(torch.isnan(ys[mesh, v])) and int(torch.isnan(xs).sum()) == 1
        P = [p.clone() for p in case.P]
        for p in P:
            p[mesh, v] = 0
        for form in POOL_FORMS:
            what = "pooling, %s in vertex %d of mesh %d, %s headroom %d maps %s" % (value, v, mesh, shape, form[0], form[1])
            feats, gv, gmaps = _pool_run(gpu, verts, case.cams, case.maps, case.grad_out, *form)
            cf, cgv, _ = case.clean[form]
            assert _rows_differing(feats, cf) <= {(mesh, v)} and _rows_differing(gv, cgv) <= {(mesh, v)}, what
            if mesh == 0:     # (vertex 100 of mesh 1 lies outside that camera's image: its clean rows are zero already)
                assert _rows_differing(feats, cf) == {(mesh, v)} and _rows_differing(gv, cgv) == {(mesh, v)}, what
            assert bool((feats[mesh, v] == 0).all()) and bool((gv[mesh, v] == 0).all()), what
            if form[1]:
                case.map_gradient_close(gmaps, P, case.grad_out, what)
        # texel 0 of one channel of every map not finite: the row holds 0 * that texel there
        maps = [t.clone() for t in case.maps]
        for t in maps:
            t[mesh, 1, 0, 0] = NAN
            t[mesh, 2, 0, 0] = INF
        feats, gv, _ = _pool_run(gpu, verts, case.cams, maps, case.grad_out, 0, True)
        want = torch.cat([nh.pool_forward64(t, *nh.pool_weights64(verts, *case.host_cams, d)[:2]) for t, d in zip(maps, case.dims)], -1)
        assert int(torch.isnan(want[mesh, v]).sum()) == 2 * len(maps) and bool((want[mesh, v][~torch.isnan(want[mesh, v])] == 0).all())
        nonfinite_close(feats[mesh, v], want[mesh, v], torch.zeros_like(want[mesh, v]), MAP_RTOL, "pooled row at a non-finite texel 0")
        assert bool((gv[mesh, v] == 0).all())


@pytest.mark.parametrize("k", [0, 1, 2])
def test_pooling_with_a_nan_camera_parameter(gpu, pool_cases, k):
    """img_info[1, k] = NaN through utils.batch_camera_info: the camera of mesh 1 is non-finite exactly where the torch
    expressions of test_camera_kernel_against_the_torch_expressions are (kinds included), mesh 0's is bit-identical; mesh 0 is
    bit-identical in the features and verts.grad and within the finite bound in the map gradients; every vertex of mesh 1 follows
    the NaN rule: zero features, zero verts.grad, nothing in any map gradient (all of mesh 1's are exactly zero)."""
    case = pool_cases["four_maps"]
    info = case.img_info.clone()
    info[1, k] = NAN
    cams = utils.batch_camera_info(info.to(gpu))
    ref = utils.batch_camera_info(info.to(gpu).requires_grad_(True))                 # the torch expressions
    for got, want, clean in zip(cams, ref, case.cams):
        assert _same_bits(got[0], clean[0])
        nonfinite_close(got[1], want[1].detach().double(), want[1].detach().double().abs().nan_to_num(0, 0, 0) + 1, 2e-6, "camera")
    assert bool(torch.isnan(cams[0][1]).all()) and bool(torch.isnan(cams[1][1]).any())
    P = [p.clone() for p in case.P]
    for p in P:
        p[1] = 0
    for form in POOL_FORMS:
        what = "pooling, NaN camera parameter %d, headroom %d maps %s" % (k, *form)
        feats, gv, gmaps = _pool_run(gpu, case.verts, cams, case.maps, case.grad_out, *form)
        cf, cgv, _ = case.clean[form]
        assert _same_bits(feats[0], cf[0]) and _same_bits(gv[0], cgv[0]), what
        assert bool((feats[1] == 0).all()) and bool((gv[1] == 0).all()), what
        if form[1]:
            case.map_gradient_close(gmaps, P, case.grad_out, what)
            assert all(bool((g[1] == 0).all()) for g in gmaps), what


def _texel_choices(case, l):
    """(mesh, texel, vertex) for the three ways of the issue, from the float64 tables of map l: (a) a texel a kept vertex reads with
    non-zero weight; (b) a texel a kept vertex reads with ZERO weight only (a clamped coordinate); (c) the pair partner of a
    clamped kept vertex's texel, which that vertex does not read."""
    index, weight, _ = case.tables[l]
    dim = case.dims[l]
    out = {}
    for mesh in range(2):
        for v in range(index.shape[1]):
            if not case.keep[mesh, v]:
                continue
            w, ix = weight[mesh, v], index[mesh, v]
            if "a" not in out and bool((w != 0).all()):
                out["a"] = (mesh, int(ix[0]), v)
            if bool((w == 0).all()):
                out.setdefault("b", (mesh, int(ix[0]), v))
                x1, y1 = int(ix[0]) // dim, int(ix[0]) % dim
                yb = min(y1, max(dim - 2, 0))
                partner = x1 * dim + (yb if y1 != yb else yb + 1)
                if "c" not in out and partner not in ix.tolist():
                    out["c"] = (mesh, partner, v)
    assert sorted(out) == ["a", "b", "c"], out
    return out


@pytest.mark.parametrize("value", ["nan", "+inf"])
@pytest.mark.parametrize("way", ["a", "b", "c"])
@pytest.mark.parametrize("shape", sorted(RAGGED_SHAPES))
def test_pooling_with_a_non_finite_texel(gpu, pool_cases, shape, way, value):
    """One texel of the last channel of one map NaN / +Inf.  Features against ref_ops.pool_features in float64, kinds=True, on the
    vertices at least POOL_NEAR from every texel line (the finite bound: 8 eps of the row's term mass, test_pooling_at_ragged_
    shapes_per_element's, + POOL_P_ULPS eps dim of every texel read, test_projection_and_weights_against_float64's); every row that
    does not read the texel in float64 is bit-identical to the clean run -- for way (c) that is the clamped vertex itself, whose
    paired read loads the texel.  verts.grad against ref_ops.pool_vertex_gradient (kinds=True for NaN; for Inf the chain forms
    Inf - Inf: the mask alone), rows that do not read the texel bit-identical to the clean run."""
    case = pool_cases[shape]
    l = POOL_PLANT_MAP[shape]
    mesh, texel, v = _texel_choices(case, l)[way]
    dim, ch = case.dims[l], case.chans[l] - 1
    maps = [t.clone() for t in case.maps]
    maps[l][mesh, ch, texel // dim, texel % dim] = nh.VALUES[value]
    index, weight, _ = case.tables[l]
    readers = {(mesh, int(u)) for u in torch.nonzero((index[mesh] == texel).any(-1)).flatten()}
    assert ((mesh, v) in readers) == (way != "c")
    if way == "b":
        assert bool((weight[mesh, v] == 0).all())
    want = ref_ops.pool_features([t.double() for t in maps], case.verts.double(), *(t.double() for t in case.host_cams))
    mass = torch.cat([nh.pool_forward64(torch.nan_to_num(t, 0.0, 0.0, 0.0).abs(), ix, w.abs()) * MAP_RTOL
                      + POOL_P_ULPS * EPS * d * nh.pool_forward64(torch.nan_to_num(t, 0.0, 0.0, 0.0).abs(), ix, torch.ones_like(w))
                      for t, d, (ix, w, _) in zip(maps, case.dims, case.tables)], -1) / MAP_RTOL
    col = int(case.cols[l]) + ch
    assert {(int(b), int(u)) for b, u in torch.nonzero(~torch.isfinite(want).all(-1))} == readers
    assert bool((~torch.isfinite(want[mesh, [u for _, u in sorted(readers)], col])).all())
    grad64, gmass, gfloor, _ = ref_ops.pool_vertex_gradient(maps, case.verts, *case.host_cams, case.grad_out)
    gmass = np.nan_to_num(gmass, nan=0.0, posinf=0.0, neginf=0.0) + np.nan_to_num(gfloor, nan=0.0, posinf=0.0, neginf=0.0) * POOL_FLOOR_ULPS / POOL_ROW_RTOL
    keep = torch.from_numpy(case.keep)
    kept_readers = {r for r in readers if case.keep[r]}
    for form in POOL_FORMS:
        what = "pooling, %s texel (%s), %s headroom %d maps %s" % (value, way, shape, form[0], form[1])
        feats, gv, _ = _pool_run(gpu, case.verts, case.cams, maps, case.grad_out, *form)
        cf, cgv, _ = case.clean[form]
        nonfinite_close(feats[keep], want[keep], mass[keep], MAP_RTOL, what + ": features", kinds=True)
        changed = {r for r in _rows_differing(feats, cf) if case.keep[r]}
        assert changed == kept_readers, what
        assert _differing(feats[mesh, v].flatten(), cf[mesh, v].flatten()) == ([col] if way != "c" else []), what
        nonfinite_close(gv[keep], grad64[case.keep], gmass[case.keep], POOL_ROW_RTOL, what + ": verts.grad", kinds=(value == "nan"))
        assert {r for r in _rows_differing(gv, cgv) if case.keep[r]} <= kept_readers, what


@pytest.mark.parametrize("value", ["nan", "+inf"])
@pytest.mark.parametrize("shape", sorted(RAGGED_SHAPES))
def test_pooling_with_a_non_finite_output_gradient_element(gpu, pool_cases, shape, value):
    """One element of the output gradient NaN / +Inf, at a vertex with four non-zero weights and at a vertex the clamp holds on one
    axis (all four weights zero).  The map gradient is non-finite exactly at the texels the vertex holds with NON-ZERO weight, in
    that channel -- the float64 sum over the stored entries (nh.pool_map_gradient64; the dense form poisons a superset, host
    test), kinds=True -- and nowhere for the clamped vertex; every other element meets the finite test's bound against the
    kernel's own P.  The vertex's verts.grad row is non-finite, every other row and every feature bit-identical to the clean run."""
    case = pool_cases[shape]
    l = POOL_PLANT_MAP[shape]
    index, weight, _ = case.tables[l]
    dim, c, ch = case.dims[l], case.chans[l], case.chans[l] - 1
    col = int(case.cols[l]) + ch
    mesh, _, inner = _texel_choices(case, l)["a"]
    _, _, _, xs, ys = ref_ops._pool_project(case.verts.double(), *(t.double() for t in case.host_cams))
    inside = torch.stack(((xs * dim >= 0) & (xs * dim <= dim - 1), (ys * dim >= 0) & (ys * dim <= dim - 1)), -1)[mesh]
    one_axis = [u for u in range(101) if case.keep[mesh, u] and int(inside[u].sum()) == 1]
    assert one_axis and bool((weight[mesh, one_axis[0]] == 0).all()), "no vertex held on one axis only"
    for v, stored in ((inner, 4), (one_axis[0], 0)):
        grad_out = case.grad_out.clone()
        grad_out[mesh, v, col] = nh.VALUES[value]
        want, wmass = nh.pool_map_gradient64(grad_out[..., case.cols[l]:case.cols[l + 1]], index, weight, dim)
        texels = sorted(int(t) for t, w in zip(index[mesh, v], weight[mesh, v]) if w != 0)
        assert len(texels) == stored
        reach = torch.zeros(2, c, dim * dim, dtype=torch.bool)
        reach[mesh, ch, texels] = True
        reach = reach.view(2, c, dim, dim)
        assert bool(((~torch.isfinite(want)) == reach).all()), "the float64 sum over the stored entries has another reach"
        assert sorted(torch.nonzero(case.P[l][mesh, v]).flatten().tolist()) == texels, "the kernel's P holds other texels"
        finite_g = grad_out.clone()
        finite_g[mesh, v, col] = 0
        for form in POOL_FORMS:
            what = "pooling, %s output gradient at vertex %d, %s headroom %d maps %s" % (value, v, shape, form[0], form[1])
            feats, gv, gmaps = _pool_run(gpu, case.verts, case.cams, case.maps, grad_out, *form)
            cf, cgv, _ = case.clean[form]
            assert _same_bits(feats, cf), what
            assert _rows_differing(gv, cgv) == {(mesh, v)} and not bool(torch.isfinite(gv[mesh, v]).any()), what
            if not form[1]:
                continue
            got = gmaps[l].detach().cpu()
            assert bool(((~torch.isfinite(got)) == reach).all()), what + ": the non-finite texels"
            if stored:      # kinds inside the reach: +Inf stays +Inf (the weights are positive), NaN stays NaN
                nonfinite_close(got[reach], want[reach], torch.zeros_like(want[reach]), MAP_RTOL, what + ": kinds", kinds=True)
            # outside it: the finite test's reference and bound (P^T g with the kernel's own P), the planted element taken out
            finite = [g.detach().cpu().clone() for g in gmaps]
            finite[l][reach] = 0
            P = [q.clone() for q in case.P]
            refs = []
            for k, (ck, dk) in enumerate(zip(case.chans, case.dims)):
                gl = finite_g.double()[..., case.cols[k]:case.cols[k + 1]]
                ref = torch.einsum("bvt,bvc->bct", P[k], gl).view(2, ck, dk, dk)
                mass = torch.einsum("bvt,bvc->bct", P[k].abs(), gl.abs()).view(2, ck, dk, dk)
                if k == l:
                    ref[reach] = 0
                nonfinite_close(finite[k], ref, mass, MAP_RTOL, "%s, map %d x %d" % (what, dk, dk))


# ---- D. the ragged losses (ops.RaggedSurfaceLoss, ops.RaggedStageRegularisers) --------------------------------------------------
# The index paths: the ragged surface loss gathers through `choices` (given), runs the Chamfer scan (its NaN rules are pinned with
# the scans) and the culled point-to-triangle scan, whose triangle ids are loop counters that survived comparisons -- a NaN
# sphere is never culled, a NaN distance never wins, the winner goes through winner_index's clamp --, and scatters through face
# corners.  The regulariser kernels walk the CSR, the corner lists and the mesh ids.  No position is ever an index.


def _fp64_union_gradient(rb, verts, gt, draws, two_sided):
    """test_ragged_loss_gpu._fp64_union_gradient on planted vertices: (loss, grad, mass, floor) of the mean over the meshes."""
    choices, u, v = (t.cpu().numpy() for t in draws)
    total, parts = 0.0, [np.zeros(verts.shape, np.float64) for _ in range(3)]
    for m in range(rb.b):
        ids, faces_m = rb.faces_of(m)
        local = np.searchsorted(ids, choices[m])
        with np.errstate(invalid="ignore"):
            loss, *gmf = fp64_surface_gradient(verts[None], faces_m, gt[m:m + 1], local[None], u[m:m + 1], v[m:m + 1], two_sided)
        total += loss / rb.b
        for acc, x in zip(parts, gmf):
            acc += x[0] / rb.b
    return (total,) + tuple(parts)


@pytest.mark.parametrize("touched", [True, False], ids=["drawn", "not_drawn"])
@pytest.mark.parametrize("fn_name, two_sided", [("point_to_surface", False), ("point_to_point", True)])
def test_ragged_surface_loss_with_a_nan_vertex(gpu, ragged_a, fn_name, two_sided, touched):
    """utils.ragged_point_to_surface / ragged_point_to_point on batch_a() with replayed draws (65 samples a mesh), one NaN
    coordinate in a vertex of the 1280-face mesh -- one a drawn face touches, and one no drawn face touches.  The loss is NaN
    exactly when the mean of ref_ops' per-mesh losses on the same draws is, a finite one agrees to 1e-5 (_nan_exactly_when).
    verts.grad against the float64 term-by-term gradient (helpers.fp64_surface_gradient per mesh): non-finite at the same
    elements -- the corners of the faces that carry a non-finite term --, every other element within the finite test's bound
    (ROW_RTOL_SURFACE, ROW_FLOOR_ULPS: the backward scatters with fp32 atomics, its summation order is not fixed, so the rows are
    not bit-identical from run to run, and no comparison with a clean run is made; kinds=False: a corner's sum may hold NaN
    terms of either sign).  The vertex is not taken from the mesh's FIRST face: a NaN first triangle seeds every query's arg-min
    ("the NaN seed sticks") and the whole mesh's term is NaN -- that rule is pinned where the scans are
    (test_scan_parity_gpu.py: the degenerate first triangle; test_ragged_loss_gpu.py::test_scan_is_the_per_mesh_scan holds the
    ragged scan to the per-mesh one bit for bit), not here."""
    d, rb, mesh, num, n_gt = ragged_a, ragged_a.rb, 1, 65, 65
    gt_np = meshgen.gt_cloud(rb.b, n_gt, first=5)
    gt = _to(gt_np, gpu)
    draws = ops.draw_samples_ragged(d.verts, d.faces, d.face_list, d.face_off, num, generator=torch.Generator(device=gpu).manual_seed(86))
    ids, faces_m = rb.faces_of(mesh)
    drawn = set(rb.faces[draws[0][mesh].cpu().numpy()].reshape(-1).tolist())
    pool = sorted(set(faces_m[1:].reshape(-1).tolist()) - set(faces_m[0].tolist()))     # (not the mesh's first face: its NaN seed sticks)
    v = next(x for x in pool if (x in drawn) == touched)
    planted = nh.planted_vertex(rb.verts, v, NAN)
    verts = _to(planted, gpu).requires_grad_(True)
    loss = getattr(utils, "ragged_" + fn_name)(verts, d.faces, d.face_mesh, gt, num=num, draws=draws)
    loss.backward()
    cpu = lambda t: t.detach().cpu()
    ref_fn = ref_ops.point_to_point if two_sided else ref_ops.point_to_surface
    refs = []
    for m in range(rb.b):
        ids_m, f_m = rb.faces_of(m)
        local = torch.from_numpy(np.searchsorted(ids_m, cpu(draws[0][m]).numpy()))[None]
        refs.append(ref_fn(torch.from_numpy(planted)[None], torch.from_numpy(f_m), cpu(gt[m:m + 1]), local, cpu(draws[1][m:m + 1]),
                           cpu(draws[2][m:m + 1])))
    ref = torch.stack([r.double() for r in refs]).mean()
    assert _nan_exactly_when(loss, ref, "ragged_" + fn_name) == touched, "the restatement is %sNaN" % ("not " if touched else "")
    exact_loss, grad, mass, floor = _fp64_union_gradient(rb, planted, gt_np, draws, two_sided)
    assert np.isnan(exact_loss) == np.isnan(float(ref))
    if touched:
        assert np.isnan(float(loss)) and np.isnan(grad[v, 1])            # (the terms' gradients act coordinate by coordinate)
    bad_rows = np.flatnonzero(~np.isfinite(grad).all(-1))
    assert set(bad_rows.tolist()) <= set(faces_m[(faces_m == v).any(1)].reshape(-1).tolist()) | {v}
    fin = lambda a: np.where(np.isfinite(a), a, 0.0)
    nonfinite_close(verts.grad, grad, fin(mass) + fin(floor) * ROW_FLOOR_ULPS / ROW_RTOL_SURFACE, ROW_RTOL_SURFACE,
                    "ragged_%s verts.grad, NaN vertex %s" % (fn_name, "drawn" if touched else "not drawn"), kinds=False)


def _reg_weights(kind, b, mesh):
    if kind == "scalar":
        return SCALAR_WEIGHTS
    w = ([300.0 * (m + 1) for m in range(b)], [20.0 + 5.0 * m for m in range(b)], [300.0] * b)
    if kind == "zero":            # every weight of the planted mesh 0: a coefficient 0 does not drop the NaN
        for row in w:
            row[mesh] = 0.0
    return w


@pytest.mark.parametrize("which", ["cur", "prev"])
@pytest.mark.parametrize("kind", ["scalar", "per-mesh", "zero"])
@pytest.mark.parametrize("name", ["mixed", "edge-cut"])
def test_ragged_stage_regularisers_with_a_nan_vertex(gpu, name, kind, which):
    """utils.ragged_stage_regularisers with one NaN coordinate in a vertex of one mesh (in cur, in prev), scalar weights, per-mesh
    weights, and per-mesh weights that are all 0 for the planted mesh: the value is NaN exactly when ragged_reg_helpers.
    reference_value in float64 is (0 * NaN: a zero coefficient does not drop it).  grad_prev and grad_cur against the float64
    chain over the STORED adjacency entries (ref_ops.sparse_aggregate), nonfinite_close(kinds=False: the Laplacian's differences
    may form Inf - Inf / NaN of either sign): non-finite exactly in the planted COORDINATE of the vertex's two-ring (lap^T lap
    reaches the neighbours' neighbours; its faces' corners lie inside), every other element bit-identical to the clean run."""
    from test_ragged_regularisers_gpu import GOUT, OnDevice, on_device, outputs
    rb = BATCHES[name]()
    mesh = 1
    v = int(rb.vids[mesh][len(rb.vids[mesh]) // 2])
    weights = _reg_weights(kind, rb.b, mesh)
    clean = OnDevice(rb, gpu)
    base = outputs(clean, clean.loss(on_device(weights, gpu)))
    getattr(rb, which)[v, 1] = NAN
    d = OnDevice(rb, gpu)
    loss = d.loss(on_device(weights, gpu))
    got = outputs(d, loss)
    want, _, _ = reference_value(rb, weights)
    assert _nan_exactly_when(loss, want.detach(), "ragged_stage_regularisers") and np.isnan(float(loss))
    exact = union_chain(rb, weights, GOUT, aggregate=ref_ops.sparse_aggregate)
    mass = union_chain(rb, weights, GOUT, absolute=True, aggregate=ref_ops.sparse_aggregate)
    floor = union_chain(rb, weights, GOUT, absolute=True, ulps=True, aggregate=ref_ops.sparse_aggregate)
    fin = lambda t: np.nan_to_num(t.numpy(), nan=0.0, posinf=0.0, neginf=0.0)
    adj = rb.union_adj() != 0
    ring1 = adj[v]
    ring2 = (adj[ring1].any(0)).numpy()
    for key in ("grad_prev", "grad_cur"):
        e = exact[key].numpy()
        reach = ring2[:, None] & (np.arange(3) == 1)[None]                 # (every term acts coordinate by coordinate)
        assert np.array_equal(~np.isfinite(e), reach), "the float64 chain's reach is not the two-ring's coordinate (%s)" % key
        # the finite rows: the finite test's bound (ragged_reg_helpers.bounds: (row_terms + 8) * 2^-24 of the term mass + one
        # coordinate ulp per term), the longest row or corner list of any mesh
        corners = int(np.bincount(rb.faces.reshape(-1).numpy(), minlength=rb.vt).max())
        rtol = (max(int(adj.sum(1).max()), corners) + 8) * 2.0 ** -24
        nonfinite_close(got[key], e, fin(mass[key]) + fin(floor[key]) * ROW_FLOOR_ULPS / rtol, rtol,
                        "ragged regularisers %s %s %s, NaN in %s" % (name, kind, key, which), kinds=False)
        assert np.array_equal(got[key][~reach].view(np.uint32), base[key][~reach].view(np.uint32)), key + ": an element outside the reach changed"

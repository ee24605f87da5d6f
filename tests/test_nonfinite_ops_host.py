"""Host side of tests/test_nonfinite_ops_gpu.py: the restatements the kernels are held to with a NaN or
an Inf planted, checked against float64 where float64 is defined, and each reach assertion SHOWN TO BITE on a planted fault of
the restatement (never of a kernel):

  * the sampler: a face whose fp32 area is NaN weighs nothing and every other face keeps its share -- the table of an
    unconditional `run += area` loses every face behind the first NaN one;
  * Adam: the written rule gives m = +-Inf, v = +Inf and the update Inf / Inf = NaN for an infinite gradient, as
    torch.optim.Adam in float64 does -- an update that skips a non-finite gradient leaves finite values behind;
  * the pooling: a NaN in the output gradient reaches the texels its vertex holds with NON-ZERO weight -- the "multiply by the
    zero weight" form (autograd's) poisons a superset; a vertex whose projection is NaN adds nothing anywhere."""
import numpy as np
import pytest
import torch

import draw_helpers as dh
import nonfinite_ops_helpers as nh
from geometrics_amd import meshgen
from helpers import nonfinite_close
from oracle import ref_ops


# ---- B. the face sampler ---------------------------------------------------------------------------------------------------
def _mesh(level):
    V, F = meshgen.icosphere(level)
    return meshgen.jittered_batch(V, 1)[0], F


@pytest.mark.parametrize("level", [2, 3])
def test_sampler_plants_sit_where_they_are_meant_to(level):
    verts, faces = _mesh(level)
    nf = faces.shape[0]
    per = (nf + dh.THREADS - 1) // dh.THREADS
    assert (nf, per) == {2: (320, 1), 3: (1280, 2)}[level]
    plants = nh.sampler_plants(faces)
    assert 0 in nh.faces_of_vertex(faces, plants["low"]) and nf - 1 in nh.faces_of_vertex(faces, plants["last"])
    touched = nh.faces_of_vertex(faces, plants["boundary"])
    assert touched.min() > 0 and len({f // per for f in touched}) > 1
    if per == 2:      # a thread whose two faces are one NaN area and one that weighs
        assert any((f ^ 1) not in touched for f in touched)


@pytest.mark.parametrize("where", ["low", "boundary", "last"])
@pytest.mark.parametrize("level", [2, 3])
def test_a_nan_face_weighs_nothing_and_the_others_keep_their_share(level, where):
    """All 2^24 uniforms through the extended restatement with NaN in one vertex: no face of that vertex is drawn, and every
    other face's count lies within K = draw_helpers.count_bound (test_draw_exact_host.py's bound) of the float64 inverse CDF
    over the REMAINING faces.  The unconditional running sum (the kernel up to this test) fails both on the same input."""
    verts, faces = _mesh(level)
    nf = faces.shape[0]
    v = nh.sampler_plants(faces)[where]
    planted = nh.planted_vertex(verts, v, nh.NAN)
    touched = nh.faces_of_vertex(faces, v)
    a32 = dh.face_areas_f32(planted, faces)
    assert np.isnan(a32[touched]).all() and np.isfinite(np.delete(a32, touched)).all()
    ref = dh.sweep_counts_f64(nh.remaining_areas_f64(planted, faces))
    assert (ref[touched] == 0).all() and (np.delete(ref, touched) > 0).all()
    r0 = (np.arange(dh.GRID, dtype=np.uint32).astype(np.float32) * np.float32(dh.U)).astype(np.float32)
    K = dh.count_bound(nf)

    def counts_of(tab):
        return np.bincount(dh.search(tab, dh.search_targets(tab, r0)), minlength=nf)

    tab = dh.table(a32)
    assert np.isfinite(tab).all() and (np.diff(tab) >= 0).all()
    counts = counts_of(tab)
    assert (counts[touched] == 0).all(), "a face of the NaN vertex is drawn"
    worst = int(np.abs(counts - ref).max())
    print("level %d %s: K %d, worst count difference %d" % (level, where, K, worst))
    assert worst <= K
    # the planted fault: every area added to the running sum
    lost = counts_of(nh.unconditional_table(a32))
    behind = (np.arange(nf) > touched.min()) & (np.arange(nf) < nf - 1)         # (the search's clamp ends on the last face)
    if where != "last":
        assert (lost[behind] == 0).all() and np.abs(lost - ref).max() > K, "the unconditional running sum passes"
    else:             # (the last face of the last thread that owns one: nothing lies behind it, only its own thread's sum is lost)
        assert touched.max() == nf - 1


@pytest.mark.parametrize("level", [2, 3])
def test_an_infinite_vertex_keeps_every_choice_in_range(level):
    """+Inf in a vertex: its faces' areas are +Inf or NaN (Inf - Inf in the cross product), the table holds Inf from the first
    infinite face that weighs on, the target is Inf (NaN for a uniform of 0) and the search ends on the last face.  Stated in
    DESIGN.md; here: the restatement stays inside [0, nf) and is what it is for every uniform."""
    verts, faces = _mesh(level)
    nf = faces.shape[0]
    for where, v in nh.sampler_plants(faces).items():
        planted = nh.planted_vertex(verts, v, nh.INF)
        a32 = dh.face_areas_f32(planted, faces)
        touched = nh.faces_of_vertex(faces, v)
        assert not np.isfinite(a32[touched]).any() and np.isposinf(a32[touched]).any()
        tab = dh.table(a32)
        assert not np.isnan(tab).any() and (tab[1:] >= tab[:-1]).all()
        r0 = np.linspace(0, 1, 4097, dtype=np.float32)[:-1]
        choices = dh.search(tab, dh.search_targets(tab, r0))
        assert choices.min() >= 0 and choices.max() < nf
        if np.isposinf(tab[-1]):
            assert (choices == nf - 1).all(), where


# ---- C. Adam ---------------------------------------------------------------------------------------------------------------
def _adam_case(value, where="grad"):
    rng = np.random.default_rng(5)
    params = [rng.standard_normal(n) for n in (1, 7, 1025)]
    clean = [[rng.standard_normal(p.shape) for p in params] for _ in range(3)]
    grads = [[g.copy() for g in step] for step in clean]
    if where == "grad":
        for step in grads[:2]:
            step[2][1024] = value
    else:
        params[2][1024] = value
    return params, clean, grads


@pytest.mark.parametrize("value", ["+inf", "-inf", "nan"])
def test_float64_adam_carries_a_non_finite_gradient_into_p_m_and_v(value):
    """What float64 gives, not a guess: after the first step with g = +-Inf, m = +-Inf, v = +Inf and p = NaN (Inf / Inf), in
    torch.optim.Adam and in the written rule alike; with g = NaN all three are NaN.  On the later steps p stays NaN and v
    non-finite in both; torch forms m by lerp (m + (1 - b1) (g - m)), which is Inf - Inf = NaN from the second step on, where the
    written rule b1 m + (1 - b1) g (csrc/adam_math.h) keeps +-Inf: the KIND of m is indeterminate there, its mask is not.
    Every other element equals the clean run's."""
    x = nh.VALUES[value]
    params, clean, grads = _adam_case(x)
    rule, ref, base = nh.adam_rule64(params, grads), nh.adam_torch64(params, grads), nh.adam_torch64(params, clean)
    for step, (a, b, c) in enumerate(zip(rule, ref, base)):
        for name, ra, rb, rc in zip(("p", "m", "v"), a, b, c):
            for i in range(3):
                if name != "m" or step == 0 or value == "nan":        # (m behind an infinite gradient: torch's lerp, see above)
                    np.testing.assert_allclose(ra[i], rb[i], rtol=1e-12, atol=1e-300, equal_nan=True)
                assert np.array_equal(np.isfinite(ra[i]), np.isfinite(rb[i]))
                reach = np.zeros(ra[i].shape, bool)
                reach[1024 if i == 2 else slice(0, 0)] = True
                assert np.array_equal(~np.isfinite(rb[i]), reach), "the reach of the planted gradient in %s" % name
                assert np.array_equal(rb[i][~reach], rc[i][~reach])
        p, m, v = (t[2][1024] for t in a)
        if value == "nan":
            assert np.isnan(p) and np.isnan(m) and np.isnan(v)
        else:
            assert np.isnan(p) and m == x and v == nh.INF
            assert np.isnan(b[0][2][1024]) and b[2][2][1024] == nh.INF and (b[1][2][1024] == x if step == 0 else not np.isfinite(b[1][2][1024]))


def test_a_non_finite_parameter_stays_alone():
    for x in (nh.NAN, nh.INF):
        params, clean, _ = _adam_case(x, "param")
        ref, rule = nh.adam_torch64(params, clean), nh.adam_rule64(params, clean)
        for (p, m, v), (rp, rm, rv) in zip(ref, rule):
            assert not np.isfinite(p[2][1024]) and np.isfinite(np.delete(p[2], 1024)).all() and np.isfinite(m[2]).all() and np.isfinite(v[2]).all()
            np.testing.assert_allclose(rp[2], p[2], rtol=1e-12, equal_nan=True)


def test_an_adam_that_skips_non_finite_gradients_is_caught():
    """The comparison the GPU test makes (helpers.nonfinite_close against float64 torch.optim.Adam) on the written rule, and on
    the planted fault -- an update that leaves an element alone whose gradient is not finite: finite where float64 is not."""
    for value in ("nan", "+inf"):
        params, _, grads = _adam_case(nh.VALUES[value])
        ref = nh.adam_torch64(params, grads)
        for skip in (False, True):
            got = nh.adam_rule64(params, grads, skip_nonfinite=skip)

            def compare():
                for (gp, gm, gv), (rp, rm, rv) in zip(got, ref):
                    for g, r in ((gp, rp), (gv, rv), (gm, rm)):
                        nonfinite_close(g[2].astype(np.float32), r[2], nh.adam_mass(r[2]), nh.ADAM_RTOL, "adam", kinds=False)
            if skip:
                with pytest.raises(AssertionError, match="finite on one side only"):
                    compare()
            else:
                compare()


# ---- A. the pooling --------------------------------------------------------------------------------------------------------
def _pool_inputs():
    from geometrics_amd import utils
    V, _ = meshgen.icosphere(1)
    V = np.concatenate([V, 0.5 * V, 2.5 * V], 0)[:101]              # test_pooling_vertex_gradient_gpu.ragged_inputs()
    verts = torch.from_numpy(meshgen.jittered_batch(V, 2))
    cams = utils.batch_camera_info(torch.tensor([[35.0, 20.0, 1.2], [250.0, -30.0, 0.8]]))
    gen = torch.Generator().manual_seed(32)
    maps = [torch.randn(2, c, d, d, generator=gen) for c, d in ((5, 9), (3, 2), (4, 1))]
    return verts, cams, maps, torch.randn(2, 101, 12, generator=gen)


def test_the_pooling_rule_is_the_reference_on_finite_vertices_and_texel_0_on_nan_ones():
    """nh.pool_weights64 / pool_forward64 (the rule the GPU test holds a NaN vertex to) equal ref_ops.pool_features wherever the
    projection is finite -- with a NaN and an Inf texel in the maps too: 0 * NaN is formed by both -- and put a vertex whose
    projection is NaN at texel 0 with four zero weights.  +-Inf in a coordinate projects to NaN as well (Inf / Inf)."""
    verts, cams, maps, _ = _pool_inputs()
    maps[0][0, 1, 3, 4], maps[0][1, 2, 0, 0], maps[1][1, 0, 0, 0] = nh.NAN, nh.INF, nh.NAN
    want = ref_ops.pool_features([m.double() for m in maps], verts.double(), *(c.double() for c in cams))
    got = torch.cat([nh.pool_forward64(m, *nh.pool_weights64(verts, *cams, m.shape[-1])[:2]) for m in maps], -1)
    assert not bool(torch.isfinite(want).all())
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-12, atol=1e-15, equal_nan=True)
    for value in (nh.NAN, nh.INF, -nh.INF):
        planted = verts.clone()
        planted[1, 100, 1] = value
        for m in maps:
            index, weight, nan = nh.pool_weights64(planted, *cams, m.shape[-1])
            assert bool(nan[1, 100]) and int(nan.sum()) == 1
            assert index[1, 100].tolist() == [0, 0, 0, 0] and weight[1, 100].tolist() == [0.0, 0.0, 0.0, 0.0]
        got = torch.cat([nh.pool_forward64(m, *nh.pool_weights64(planted, *cams, m.shape[-1])[:2]) for m in maps], -1)
        others = torch.ones(2, 101, dtype=torch.bool)
        others[1, 100] = False
        np.testing.assert_allclose(got[others].numpy(), want[others].numpy(), rtol=1e-12, atol=1e-15, equal_nan=True)
        row = got[1, 100]
        assert torch.nonzero(torch.isnan(row)).flatten().tolist() == [2, 5] and bool((row[~torch.isnan(row)] == 0).all())


def test_the_map_gradient_is_a_sum_over_stored_corners_and_the_dense_form_poisons_a_superset():
    """A NaN in the output gradient of a vertex: the sum over the corners of NON-ZERO weight (what corners() of csrc/pooling.hip
    lists) is NaN at those texels in that channel; the "multiply by the zero weight" form -- autograd's gradient of the
    reference's expression -- is NaN at every corner the vertex reads, a superset: strictly larger for a vertex the clamp holds on
    one axis (four zero weights, none stored).  On finite gradients the two agree with autograd."""
    verts, cams, maps, grad_out = _pool_inputs()
    leaves = [m.double().requires_grad_(True) for m in maps]
    feats = ref_ops.pool_features(leaves, verts.double(), *(c.double() for c in cams))
    auto = torch.autograd.grad(feats, leaves, grad_out.double(), retain_graph=True)
    index, weight, _ = nh.pool_weights64(verts, *cams, 9)
    for stored_only in (True, False):
        got, _ = nh.pool_map_gradient64(grad_out[..., :5], index, weight, 9, stored_only)
        np.testing.assert_allclose(got.numpy(), auto[0].numpy(), rtol=1e-12, atol=1e-14)
    held = [v for v in range(101) if bool((weight[0, v] == 0).all())]
    inner = [v for v in range(101) if bool((weight[0, v] != 0).all())]
    assert held and inner
    for v, stored in ((inner[0], 4), (held[0], 0)):
        g = grad_out.clone()
        g[0, v, 3] = nh.NAN
        sparse, mass = nh.pool_map_gradient64(g[..., :5], index, weight, 9)
        dense, _ = nh.pool_map_gradient64(g[..., :5], index, weight, 9, stored_only=False)
        auto = torch.autograd.grad(feats, leaves, g.double(), retain_graph=True)[0]
        bad_sparse, bad_dense = torch.isnan(sparse), torch.isnan(dense)
        assert int(bad_sparse.sum()) == stored and bool((bad_dense | ~bad_sparse).all())
        assert bool((torch.isnan(auto) == bad_dense).all()), "autograd's reach is the dense form's"
        assert bool(torch.isfinite(mass).all())
        nonfinite_close(sparse.float(), sparse, mass, 8 * 2.0 ** -23, "map gradient")
        if not stored:      # the comparison of the GPU test, on the planted fault: finite on one side only
            assert int(bad_dense.sum()) > 0
            with pytest.raises(AssertionError, match="finite on one side only"):
                nonfinite_close(dense.float(), sparse, mass, 8 * 2.0 ** -23, "map gradient")


def test_the_float64_vertex_gradient_treats_the_clamp_as_a_select():
    """ref_ops.pool_vertex_gradient with a NaN texel: a vertex the clamp holds on both axes keeps an exactly zero row (and a
    finite mass) although it reads the texel -- torch's clamp backward is a select, and so is the kernel's `if (t.in_x)`."""
    verts, cams, maps, grad_out = _pool_inputs()
    clean = ref_ops.pool_vertex_gradient(maps, verts, *cams, grad_out)
    _, _, _, xs, ys = ref_ops._pool_project(verts.double(), *(c.double() for c in cams))
    held = ((xs * 9 < 0) | (xs * 9 > 8)) & ((ys * 9 < 0) | (ys * 9 > 8))
    zero_rows = np.argwhere(held.numpy() & (clean[0] == 0).all(-1))
    assert len(zero_rows)
    b, v = zero_rows[0]
    index, _, _ = nh.pool_weights64(verts, *cams, 9)
    t = int(index[b, v, 0])
    maps[0][b, 2, t // 9, t % 9] = nh.NAN
    grad, mass, floor, _ = ref_ops.pool_vertex_gradient(maps, verts, *cams, grad_out)
    assert (grad[b, v] == 0).all() and (mass[b, v] == 0).all() and (floor[b, v] == 0).all()
    assert np.array_equal(np.isnan(grad).any(-1), np.isnan(mass).any(-1))
    same = ~np.isnan(grad)
    np.testing.assert_array_equal(grad[same], clean[0][same])

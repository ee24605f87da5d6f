"""-m gpu: the face sampler (csrc/draw_body.h) draw for draw.  Its three launches -- geom_draw_samples_f32 (uniforms given),
geom_draw_samples_rng_f32 (in-kernel Philox) and the fused geom_surface_prepare_f32 -- against the host restatement of
tests/draw_helpers.py, BIT FOR BIT: which face every one of the 2^24 values of a uniform selects, that the stream is
Philox4x32-10 with the documented counter and key layout (also where the seed, the mesh offset and the stream position have
high bits set), and that a face of zero area is never drawn.  The restatement itself is held to the float64 inverse CDF in
tests/test_draw_exact_host.py; the statistical tests (test_sampler_statistics_gpu.py) stay what they are."""
import functools

import numpy as np
import pytest
import torch

import draw_helpers as dh
from geometrics_amd import _lib, meshgen, ops

pytestmark = pytest.mark.gpu

HIGH_SEED = 0x1234_5678_9ABC_DEF0 & (2 ** 63 - 1)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _to(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _given(gpu, verts, faces, uniforms):
    """geom_draw_samples_f32 on uniforms laid out [3, B, num]: (choices, u, v) as numpy."""
    _, b, num = uniforms.shape
    choices = torch.empty(b, num, dtype=torch.int64, device=gpu)
    u = torch.empty(b, num, dtype=torch.float32, device=gpu)
    v = torch.empty(b, num, dtype=torch.float32, device=gpu)
    _lib.call("geom_draw_samples_f32", b, verts.shape[1], _to(verts, gpu), faces.shape[0], _to(faces, gpu), num, _to(uniforms, gpu),
              choices, u, v)
    return choices.cpu().numpy(), u.cpu().numpy(), v.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _sweep_uniforms():
    """[3, 1, 2^24]: r0 = every value a 24-bit uniform takes, ascending; r1, r2 = two fixed scrambles of the same grid."""
    k = np.arange(dh.GRID, dtype=np.uint64)
    grid = lambda x: ((x % np.uint64(dh.GRID)).astype(np.float32) * np.float32(dh.U)).astype(np.float32)
    return np.stack([grid(k), grid(k * np.uint64(2654435761) + np.uint64(12345)), grid(k * np.uint64(40503) + np.uint64(977))])[:, None, :]


@pytest.mark.parametrize("nf", [20, 1023, 1025, 16384])
def test_every_uniform_selects_the_restated_face(gpu, nf):
    """One mesh, all 2^24 values of r0 in one call (16384 workgroups, each rebuilding the table): choices, u and v bit-equal to
    the restatement for every sample, no zero-area face (one face in ten is one), non-decreasing in r0, and per-face counts
    within K = draw_helpers.count_bound of the float64 inverse CDF's (K = 60 / 60 / 62 / 90, derived there; measured worst
    difference 2 / 3 / 3 / 3.  The scanned sums without the running maximum, the kernel up to this test: 1 / 12 / 8 / 11
    uniforms draw a zero-area face.)"""
    verts, faces = dh.triangle_soup(nf, 1000 + nf)
    uniforms = _sweep_uniforms()
    choices, u, v = _given(gpu, verts[None], faces, uniforms)
    ref_c, ref_u, ref_v, _ = dh.draw(verts, faces, uniforms[0, 0], uniforms[1, 0], uniforms[2, 0])
    differ = np.flatnonzero(choices[0] != ref_c)
    assert differ.size == 0, "%d uniforms select another face than restated, first k = %s: %s against %s" % (
        differ.size, differ[:4], choices[0][differ[:4]], ref_c[differ[:4]])
    assert np.array_equal(_bits(u[0]), _bits(ref_u)) and np.array_equal(_bits(v[0]), _bits(ref_v))
    a64 = dh.face_areas_f64(verts, faces)
    assert (a64 == 0).sum() >= nf // 10 and not (a64[choices[0]] == 0).any(), "a zero-area face was drawn"
    assert (np.diff(choices[0]) >= 0).all()
    counts, ref_counts = np.bincount(choices[0], minlength=nf), dh.sweep_counts_f64(a64)
    K = dh.count_bound(nf)
    worst = int(np.abs(counts - ref_counts).max())
    print("nf %d: K %d, worst count difference %d" % (nf, K, worst))
    assert worst <= K


def _batched_case(nf, B, level=None):
    """(verts [B, nv, 3], faces): a triangle soup (or a jittered icosphere) with positions of its own for every mesh."""
    if level is not None:
        V, faces = meshgen.icosphere(level)
        return meshgen.jittered_batch(V, B), faces
    _, faces = dh.triangle_soup(nf, 77)
    return np.stack([dh.triangle_soup(nf, 77 + 13 * m)[0] for m in range(B)]), faces      # (a repeated corner is degenerate anywhere)


@pytest.mark.parametrize("num", [1531, 1])
def test_given_uniforms_batched(gpu, num):
    """B = 3 meshes of 1025 faces with their own positions, num no multiple of 1024 (and 1): the `plane` stride of the uniforms
    and the per-mesh table.  r0 off the 24-bit grid as well."""
    B = 3
    verts, faces = _batched_case(1025, B)
    rng = np.random.default_rng(num)
    uniforms = rng.random((3, B, num), dtype=np.float32)
    uniforms[0, :, ::2] *= np.float32(0.77)                                                  # off the grid
    uniforms[0, 0, :3] = [0.0, 1 - 2.0 ** -24, np.nextafter(np.float32(1), np.float32(0))][:min(3, num)]
    choices, u, v = _given(gpu, verts, faces, uniforms)
    for m in range(B):
        ref_c, ref_u, ref_v, _ = dh.draw(verts[m], faces, uniforms[0, m], uniforms[1, m], uniforms[2, m])
        assert np.array_equal(choices[m], ref_c), "mesh %d" % m
        assert np.array_equal(_bits(u[m]), _bits(ref_u)) and np.array_equal(_bits(v[m]), _bits(ref_v))
        assert not (dh.face_areas_f64(verts[m], faces)[choices[m]] == 0).any()


def _restated_call(verts, faces, seed, position, mesh_offset, num):
    """What one call draws for every mesh at `position` of the stream: (choices, u, v, points) stacked over the meshes."""
    outs = [dh.draw(verts[m], faces, *dh.stream_uniforms(seed, position, mesh_offset + m, num)) for m in range(verts.shape[0])]
    return [np.stack([o[k] for o in outs]) for k in range(4)]


def _assert_call(got, want, what):
    choices, u, v, points = (t.cpu().numpy() for t in got[:4])
    assert np.array_equal(choices, want[0]), what + ": choices"
    assert np.array_equal(_bits(u), _bits(want[1])), what + ": u"
    assert np.array_equal(_bits(v), _bits(want[2])), what + ": v"
    assert np.array_equal(_bits(points), _bits(want[3])), what + ": points"


@pytest.mark.parametrize("seed,mesh_offset,position", [(HIGH_SEED, 0, 0), (HIGH_SEED, 5 << 24, 0), (123, 5 << 24, 0), (123, 0, (3 << 32) | 0xFFFFFFFF)],
                         ids=["high_seed", "high_seed_offset", "offset", "high_position"])
@pytest.mark.parametrize("nf", [320, 1025])
def test_in_kernel_philox_stream(gpu, nf, seed, mesh_offset, position):
    """ops.draw_samples(with_points=True) on B = 3, num = 1531, twice: positions p and p + 1 of the stream.  choices, u, v and
    points equal the restatement bit for bit -- counter (sample, mesh_offset + mesh, position low, position high), key (seed
    low, seed high), words x / y / z for the face, U1 and U2 --, and the state reads position p + 2, arrival counter 0."""
    B, num = 3, 1531
    verts, faces = _batched_case(nf, B, level=2 if nf == 320 else None)
    assert faces.shape[0] == nf
    state = ops.manual_seed(seed, gpu, mesh_offset=mesh_offset)
    try:
        state[1] = position                                  # (the stream position is the second word of the state)
        dv, df = _to(verts, gpu), _to(faces, gpu)
        for call in range(2):
            got = ops.draw_samples(dv, df, num, with_points=True)
            _assert_call(got, _restated_call(verts, faces, seed, position + call, mesh_offset, num), "call %d" % call)
        assert ops._rng_state(gpu).cpu().tolist() == [seed, position + 2, 0, mesh_offset]
    finally:
        ops.manual_seed(0, gpu)


def test_fused_prepare_falls_back_to_the_same_draws(gpu):
    """prepare_scan_for= at a shape whose scan does not take the fused route (test_sorted_draws_at_ragged_sizes: level 2, B 2, num
    500, n_gt 500): the launch makes independent draws, the same bits."""
    B, num, n_gt = 2, 500, 500
    verts, faces = _batched_case(320, B, level=2)
    dv, df, gt = _to(verts, gpu), _to(faces, gpu), _to(meshgen.gt_cloud(B, n_gt), gpu)
    ops.manual_seed(HIGH_SEED, gpu, mesh_offset=5 << 24)
    try:
        got = ops.draw_samples(dv, df, num, with_points=True, prepare_scan_for=n_gt, gt_index=ops.GtIndex(gt))
        assert not isinstance(got[4], ops.ScanPrep)
        _assert_call(got, _restated_call(verts, faces, HIGH_SEED, 0, 5 << 24, num), "fallback")
        assert ops._rng_state(gpu).cpu().tolist() == [HIGH_SEED, 1, 0, 5 << 24]
    finally:
        ops.manual_seed(0, gpu)


def test_fused_prepare_without_an_index_draws_the_same(gpu):
    """prepare_scan_for= at a step the fused scan route takes, no gt_index: draws + triangle records in one launch
    (surface_prepare_kernel), independent draws -- the same bits as the stand-alone launch."""
    B, num = 8, 3000
    V, faces = meshgen.icosphere(4)
    verts = meshgen.jittered_batch(V, B)
    ops.manual_seed(HIGH_SEED, gpu, mesh_offset=5 << 24)
    try:
        got = ops.draw_samples(_to(verts, gpu), _to(faces, gpu), num, with_points=True, prepare_scan_for=num)
        assert got[4] is not None, "the fused launch did not run"
        _assert_call(got, _restated_call(verts, faces, HIGH_SEED, 0, 5 << 24, num), "fused")
    finally:
        ops.manual_seed(0, gpu)


def test_visiting_order_route(gpu):
    """gt_index= at level 3, B 6, num 1000, n_gt 2750 (a shape of test_sorted_draws_at_ragged_sizes that generates the samples in
    visiting order), on an icosphere with 9 faces made degenerate by a repeated corner.  The face's uniform comes from __logf
    there and cannot be restated; u and v can: sqrt(u01(word y)) and u01(word z) of the restated stream, bit for bit, on two
    consecutive calls.  No zero-area face is drawn, and the faces' positions in the visiting order never decrease."""
    from geometrics_amd.tri_distance import face_order
    B, num, n_gt, seed, offset = 6, 1000, 2750, HIGH_SEED, 5 << 24
    V, faces = meshgen.icosphere(3)
    faces = faces.copy()
    flat = np.arange(5, faces.shape[0], 150)
    faces[flat, 2] = faces[flat, 0]
    verts = meshgen.jittered_batch(V, B)
    dv, df, gt = _to(verts, gpu), _to(faces, gpu), _to(meshgen.gt_cloud(B, n_gt), gpu)
    gi = ops.GtIndex(gt)
    order = face_order(dv, df).long()
    rank = torch.empty_like(order)
    rank[order] = torch.arange(order.numel(), device=gpu)
    ops.manual_seed(seed, gpu, mesh_offset=offset)
    try:
        for call in range(2):
            d = ops.draw_samples(dv, df, num, with_points=True, prepare_scan_for=n_gt, gt_index=gi)
            assert isinstance(d[4], ops.ScanPrep) and d[4].sample_index is not None, "the visiting-order generation did not run"
            pos = rank[d[0]]
            assert bool((pos[:, 1:] >= pos[:, :-1]).all())
            choices, u, v = (t.cpu().numpy() for t in d[:3])
            for m in range(B):
                _, r1, r2 = dh.stream_uniforms(seed, call, offset + m, num)
                assert np.array_equal(_bits(u[m]), _bits(np.sqrt(r1))) and np.array_equal(_bits(v[m]), _bits(r2)), "mesh %d" % m
                zero = dh.face_areas_f64(verts[m], faces) == 0
                assert zero.sum() == flat.size and not zero[choices[m]].any(), "a zero-area face was drawn"
                want = dh.sampled_points(verts[m], faces, choices[m], u[m], v[m])          # (of the face the kernel chose)
                assert np.array_equal(_bits(d[3][m].cpu().numpy()), _bits(want))
        assert ops._rng_state(gpu).cpu().tolist() == [seed, 2, 0, offset]
    finally:
        ops.manual_seed(0, gpu)

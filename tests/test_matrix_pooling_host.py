"""CPU: the projection-matrix pooling without a device -- the four entry points as the header declares
them, the limits and GEOM_EINVAL they answer before any pointer is touched, the argument checks of utils.pooling /
batched_pooling / ragged_pooling for matrices, and the float64 restatement tests/pool_matrix_ref.py pinned to the reference's
own runs (tests/golden/pooling_matrix.npz, made by tests/golden/make_matrix_pooling.py) and, for the matrices of family E, to
oracle.ref_ops.pool_features with the equivalent cameras.

Bounds the reference's fp32 run is held to (the ones tests/test_matrix_pooling_gpu.py holds the kernels to):
  * position gradient: pool_matrix_ref.vertex_gradient_close -- 8 eps of the element's term mass + 1 texel-coordinate ulp through
    every term, near-line vertices left out under the 2 % cap, exactly zero rows where float64 is exactly zero;
  * features: a feature is sum_t P[v,t] map[t], so |error| <= POOL_MATRIX_P_ULPS eps dim (|c11| + |c12| + |c21| + |c22|) -- the
    bar for an entry of P through the four texels it can move -- + 8 eps sum |P||map| for the products and the sum;
  * map gradient: P^T g with the float64 P: 8 eps sum |P||g| + POOL_MATRIX_P_ULPS eps dim sum |g| over the vertices that reach
    the texel (the reference's fp32 weights are its own; the GPU test takes the kernel's P and needs no second term).
pool_matrix_ref.POOL_MATRIX_P_ULPS = 3.9 = 4 x 0.975, the worst |P_fp32 - P_float64| in eps * dim that the restatement's own fp32 host run
reaches on the kept vertices of the three meshes x {E, G} x the maps of pool_matrix_ref.P_DIMS (at 9 x 9, G on mesh 1), derived as
POOL_P_ULPS was; measured shares of the bounds: the restatement's fp32 run reaches 0.233 of the position-gradient bound at the
worst (G, mesh 1, thin); the reference's fp32 run: see test_the_reference_fp32_run_lies_inside_the_bounds."""
import ctypes
import functools
import subprocess

import numpy as np
import pytest
import torch

import pool_matrix_ref as pm
from helpers import golden, log_margin
from geometrics_amd import _header, _lib, utils
from oracle import ref_ops

NAMES = ("geom_pool_features_proj_fwd_f32", "geom_pool_features_proj_bwd_f32", "geom_pool_features_ragged_proj_fwd_f32",
         "geom_pool_features_ragged_proj_bwd_f32")
EINVAL, ETOOBIG, EUNSUPPORTED = (_header.CONSTANTS[k] for k in ("EINVAL", "ETOOBIG", "EUNSUPPORTED"))
EPS = pm.EPS
CASES = [(f, m, "thin") for f in "EG" for m in range(3)] + [("G", 1, "two_maps")]


# ---------------------------------------------------------------- the C ABI
def test_the_four_symbols_are_declared_and_exported_and_the_abi_version_stands():
    L = _lib.lib()
    assert L.geom_abi_version() == 16 == _lib.ABI_VERSION
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, stdout=subprocess.PIPE, text=True, timeout=60).stdout
    exported = {line.split()[2] for line in out.splitlines() if len(line.split()) == 3 and line.split()[1] in "Tt"}
    for name in NAMES:
        assert name in _lib.declared_symbols() and name in exported, name
    params = lambda name: [p for p, _, _ in _header.PARAMETERS[name]]
    assert params(NAMES[0]) == ["b", "nv", "verts", "proj", "levels", "blocks", "channels", "dims", "out", "out_ld", "n_fronts", "fronts",
                                "widths", "cols", "buf", "stream"]
    assert params(NAMES[1]) == ["b", "nv", "verts", "proj", "levels", "blocks", "channels", "dims", "grad_out", "grad_ld", "grad_blocks",
                                "grad_verts", "workspace", "workspace_bytes", "stream"]
    assert params(NAMES[2]) == ["b", "vt", "verts", "vert_mesh", "vert_list", "proj", "levels", "blocks", "channels", "dims", "out", "out_ld",
                                "stream"]
    assert params(NAMES[3]) == ["b", "vt", "verts", "vert_mesh", "vert_list", "vert_off", "proj", "levels", "blocks", "channels", "dims",
                                "grad_out", "grad_ld", "grad_blocks", "grad_verts", "workspace", "workspace_bytes", "stream"]
    # each is its camera sibling with `proj` in place of `cam_mat, cam_pos`
    for name, sibling in zip(NAMES, ("geom_pool_features_fwd_fronts_f32", "geom_pool_features_bwd_ld_f32", "geom_pool_features_ragged_fwd_f32",
                                     "geom_pool_features_ragged_bwd_f32")):
        want = [p for p in _header.PARAMETERS[sibling] if p[0] != "cam_pos"]
        assert [(("proj",) + p[1:]) if p[0] == "cam_mat" else p for p in want] == list(_header.PARAMETERS[name]), name
        assert _header.PROTOTYPES[name][0] is ctypes.c_int


def calls(b, n_verts, channels, dims, pointer, proj):
    """The four entry points with `pointer` for every device pointer but the matrices and a null host array of map pointers."""
    L = _lib.lib()
    n = len(dims)
    ch, dm = (ctypes.c_int * n)(*channels), (ctypes.c_int * n)(*dims)
    p = pointer
    return (L.geom_pool_features_proj_fwd_f32(b, n_verts, p, proj, n, None, ch, dm, p, 0, 0, None, None, None, None, None),
            L.geom_pool_features_proj_bwd_f32(b, n_verts, p, proj, n, None, ch, dm, p, 0, None, p, p, 0, None),
            L.geom_pool_features_ragged_proj_fwd_f32(b, n_verts, p, p, p, proj, n, None, ch, dm, p, 0, None),
            L.geom_pool_features_ragged_proj_bwd_f32(b, n_verts, p, p, p, p, proj, n, None, ch, dm, p, 0, None, p, p, 0, None))


def test_the_limits_and_einval_come_back_before_any_pointer_is_touched():
    """Null device pointers everywhere: the codes are those of the camera pairs, in their order."""
    assert calls(2, 100, (4, 4), (65, 7), None, None)[2:] == (EUNSUPPORTED, EUNSUPPORTED)          # ragged: maps up to 64 x 64
    assert calls(64, 100, (4096,), (64,), None, None)[2:] == (ETOOBIG, ETOOBIG)                    # one buffer, 32-bit offsets
    assert calls(64, 100, (8, 4096), (7, 64), None, None)[2:] == (ETOOBIG, ETOOBIG)
    assert calls(63, 100, (4096,), (64,), None, None) == (EINVAL,) * 4                            # inside the limits: the null pointers
    assert calls(70000, 100, (4,), (7,), 16, 16) == (EINVAL,) * 4                                  # (the null array of maps comes first)
    for bad in ((-1, 100, (4,), (7,)), (2, -1, (4,), (7,)), (2, 100, (0,), (7,)), (2, 100, (4,), (0,)), (2, 100, (4,) * 9, (7,) * 9)):
        assert calls(*bad, None, None) == (EINVAL,) * 4, bad
    # a null proj is GEOM_EINVAL whatever else is handed in (16: a non-null address that is never read -- the maps' array is null)
    assert calls(2, 100, (4,), (7,), 16, None) == (EINVAL,) * 4
    # nothing to do is no error, with the matrices present: no vertices, no meshes
    assert calls(2, 0, (4,), (7,), 16, 16)[:2] == (EINVAL,) * 2                                    # (null maps array: still refused)
    assert calls(2, 100, (), (), 16, 16) == (0,) * 4                                               # no maps: nothing to launch


# ---------------------------------------------------------------- the Python argument checks
def test_the_matrix_routes_refuse_bad_arguments_before_any_launch(monkeypatch):
    def no_launch(name, *args):
        raise AssertionError("%s was called" % name)

    monkeypatch.setattr(_lib, "call", no_launch)
    monkeypatch.setattr(_lib, "status", no_launch)
    b, vt = 3, 20
    mats = torch.eye(4).repeat(b, 1, 1)
    blocks = [torch.zeros(b, 4, 7, 7), torch.zeros(b, 2, 5, 5)]
    ragged = lambda **kw: utils.ragged_pooling(**{**dict(blocks=blocks, verts_union=torch.zeros(vt, 3), vert_mesh=torch.zeros(vt, dtype=torch.int64),
                                                          img_info=mats), **kw})
    batched = lambda **kw: utils.batched_pooling(**{**dict(blocks=blocks, verts_pos=torch.zeros(b, vt, 3), img_info=mats), **kw})
    single = lambda **kw: utils.pooling(**{**dict(blocks=[t[0] for t in blocks], verts_pos=torch.zeros(vt, 3), matrix=mats[0]), **kw})
    for call in (ragged, batched):
        with pytest.raises(RuntimeError, match="\\[B,4,4\\] tensor"):
            call(img_info=mats[:, :3])                                            # wrong shape
        with pytest.raises(RuntimeError, match="\\[B,4,4\\] tensor"):
            call(img_info=mats[:, :, :3])
        with pytest.raises(RuntimeError, match="must be fp32 \\(got torch.float64\\)"):
            call(img_info=mats.double())
        # the batch size: the batched form counts the meshes, the union's batch IS the number of matrices
        with pytest.raises(RuntimeError, match="one projection matrix per mesh: got 2 for 3" if call is batched
                           else "holds 3 images, the matrices are 2"):
            call(img_info=mats[:2])
        with pytest.raises(RuntimeError, match="live on meta, the vertices on cpu"):
            call(img_info=mats.to("meta"))                                        # another device than the vertices
    with pytest.raises(RuntimeError, match="holds 2 images, the matrices are 3"):
        ragged(blocks=[blocks[0], blocks[1][:2]])
    with pytest.raises(RuntimeError, match="fp32 \\[Vt,3\\]"):
        ragged(verts_union=torch.zeros(vt, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="\\[4,4\\] tensor"):
        single(matrix=mats)                                                       # rank
    with pytest.raises(RuntimeError, match="\\[B,4,4\\] tensor"):
        single(matrix=torch.zeros(3, 4))
    with pytest.raises(RuntimeError, match="must be fp32"):
        single(matrix=mats[0].double())
    with pytest.raises(RuntimeError, match="live on meta"):
        single(matrix=mats[0].to("meta"))
    with pytest.raises(RuntimeError, match="fp32 \\[V,3\\]"):
        single(verts_pos=torch.zeros(1, vt, 3))
    with pytest.raises(RuntimeError, match="fp32 \\[C, dim, dim\\]"):
        single(blocks=[blocks[0]])                                                # a batched map
    with pytest.raises(RuntimeError, match="fp32 \\[C, dim, dim\\]"):
        single(blocks=[blocks[0][0].double()])
    with pytest.raises(RuntimeError, match="square planes"):
        single(blocks=[torch.zeros(4, 7, 6)])
    with pytest.raises(RuntimeError, match="at least one feature map"):
        single(blocks=[])
    # without a device the checks pass and the node refuses host tensors -- still before any launch
    with pytest.raises(RuntimeError, match="must live on a HIP device"):
        single()
    with pytest.raises(RuntimeError, match="must live on a HIP device"):
        batched()


# ---------------------------------------------------------------- the restatement, pinned
@functools.lru_cache(maxsize=None)
def fixture():
    return golden("pooling_matrix")


def case_inputs(g, fam, m, shape):
    key = "%s.m%d.%s" % (fam, m, shape)
    verts, proj = torch.from_numpy(g[key + ".verts"])[None], torch.from_numpy(g[key + ".proj"])[None]
    # the fixture's inputs are the ones the tests build
    assert torch.equal(verts[0], pm.meshes()[m]) and torch.equal(proj[0], pm.family(fam)[0][m]), key
    maps, cot = pm.maps_and_gradient(shape, verts.shape[1])
    return key, verts, proj, maps, cot


@pytest.mark.parametrize("fam, m, shape", CASES)
def test_the_float64_restatement_equals_the_reference_float64_run(fam, m, shape):
    """Features, position gradient and map gradients, to 1e-12 of each tensor's scale; the closed forms (pool_vertex_gradient,
    P^T g) as well as autograd through the restated forward."""
    g = fixture()
    key, verts, proj, maps, cot = case_inputs(g, fam, m, shape)
    feats, gv, gm = pm.host_run(maps, verts, proj, cot, torch.float64)
    closed_gv = pm.pool_vertex_gradient(maps, verts, proj, cot)[0]
    closed_gm = [ref for ref, _ in pm.pool_map_gradient(*pm.SHAPES[shape], verts, proj, cot)]

    def same(got, want, what):
        got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
        assert got.shape == want.shape, what
        scale = np.abs(want).max()
        assert scale > 0 or what.endswith("1 x 1 map"), what
        assert np.abs(got - want).max() <= 1e-12 * scale, "%s %s: %g of scale %g" % (key, what, np.abs(got - want).max(), scale)

    same(feats[0], g[key + ".feats64"], "features")
    same(gv[0], g[key + ".gv64"], "position gradient (autograd)")
    same(closed_gv[0], g[key + ".gv64"], "position gradient (closed form)")
    for l, (a, c) in enumerate(zip(gm, closed_gm)):
        what = "gradient of map %d" % l + (", a 1 x 1 map" if maps[l].shape[-1] == 1 else "")
        same(a[0], g["%s.gm64.%d" % (key, l)], what)
        same(c[0], g["%s.gm64.%d" % (key, l)], what)
    # the exactly zero rows of the reference's float64 gradient are exactly zero in the closed form (the clamp is a select)
    assert np.array_equal((closed_gv[0] == 0).all(-1), (g[key + ".gv64"] == 0).all(-1))
    assert int((g[key + ".gv64"] == 0).all(-1).sum()) == int(g[key + ".zero_rows"])


@pytest.mark.parametrize("fam, m, shape", CASES)
def test_the_reference_fp32_run_lies_inside_the_bounds(fam, m, shape):
    """Measured here (worst element as a share of its bound, over the seven cases): position gradient 0.233 (G, mesh 1, thin),
    features 0.170 and map gradient 0.186 (both G, mesh 1, two_maps).  The reference forms q with torch.mm and the products in its
    own order: a second fp32 evaluation next to the restatement's own, which reaches 0.233 of the position-gradient bound."""
    g = fixture()
    key, verts, proj, maps, cot = case_inputs(g, fam, m, shape)
    chans, dims = pm.SHAPES[shape]
    r = pm.vertex_gradient_close(g[key + ".gv32"][None], maps, verts, proj, cot, "reference fp32 verts.grad " + key)
    assert int((~r["keep"]).sum()) == int(g[key + ".left_out"])
    assert r["zero_checked"] >= (r["zero_rows"] - 1 if m < 2 else 0) and r["live_rows"] >= 60, r
    if m == 1:
        assert r["zero_rows"] >= 6, r                     # vertices clamped on both axes of every map
    keep = torch.from_numpy(r["keep"])
    err = (torch.from_numpy(g[key + ".feats32"])[None].double() - torch.from_numpy(g[key + ".feats64"])[None]).abs()
    share = (err / (pm.feature_bound(maps, verts, proj) + 1e-30))[keep]
    assert log_margin("reference fp32 features " + key, float(share.max()), 1.0), float(share.max())
    # map gradient: the float64 P, so the reference's own weights get the P bar -- on the kept vertices; a vertex on a texel line
    # may reach another texel in fp32: the texels the left-out vertices reach in either run are not compared
    col = 0
    for l, (c, d) in enumerate(zip(chans, dims)):
        P = pm.pool_operator(verts.double(), proj.double(), d)[0]                                     # [V, d*d]
        share = pm.map_gradient_share(g["%s.gm32.%d" % (key, l)], g["%s.gm64.%d" % (key, l)], P, cot[0, :, col:col + c], d, keep[0],
                                      pm.POOL_MATRIX_P_ULPS)
        col += c
        assert log_margin("reference fp32 gradient of map %d %s" % (l, key), share, 1.0), share


@pytest.mark.parametrize("shape", sorted(pm.SHAPES))
def test_with_the_equivalent_matrices_the_restatement_is_the_camera_restatement(shape):
    """Family E in float64 (the matrices BEFORE their rounding to fp32): pool_matrix_ref.pool_features equals
    oracle.ref_ops.pool_features given the cameras to 1e-10 of scale, on all three meshes; so does the position gradient."""
    cam_mat, cam_pos = ref_ops.camera_info(torch.tensor(pm.CAMERAS, dtype=torch.float64))
    E = pm.equivalent_matrices(cam_mat, cam_pos)
    for m, local in enumerate(pm.meshes()):
        verts = local[None].double()
        maps, cot = pm.maps_and_gradient(shape, local.shape[0])
        maps = [t.double() for t in maps]
        want = ref_ops.pool_features(maps, verts, cam_mat[m:m + 1], cam_pos[m:m + 1])
        got = pm.pool_features(maps, verts, E[m:m + 1])
        assert float((got - want).abs().max()) <= 1e-10 * float(want.abs().max()) and float(want.abs().max()) > 0
        g_want = ref_ops.pool_vertex_gradient(maps, verts, cam_mat[m:m + 1], cam_pos[m:m + 1], cot)[0]
        g_got = pm.pool_vertex_gradient(maps, verts, E[m:m + 1], cot)[0]
        assert np.abs(g_got - g_want).max() <= 1e-10 * np.abs(g_want).max()
        assert np.array_equal((g_got == 0).all(-1), (g_want == 0).all(-1))


def test_row_2_of_the_matrix_is_never_read_by_the_restatement():
    verts = pm.meshes()[0][None]
    maps, _ = pm.maps_and_gradient("thin", 101)
    proj = pm.family("E")[0][:1].clone()
    clean = pm.pool_features(maps, verts, proj)
    proj[:, 2] = float("nan")
    assert torch.equal(pm.pool_features(maps, verts, proj), clean)


def test_the_measured_weight_bar_is_four_times_the_host_run():
    """POOL_MATRIX_P_ULPS is derived, not chosen: 4 x the worst the restatement's own fp32 run reaches on the kept vertices."""
    worst = 0.0
    for fam in "EG":
        proj = pm.family(fam)[0]
        for m, local in enumerate(pm.meshes()):
            verts, M = local[None], proj[m:m + 1]
            for dims in pm.P_DIMS:
                keep = pm.kept_vertices(verts, M, dims)
                worst = max([worst] + [pm.weights_error(pm.pool_operator(verts, M, d), verts, M, d, keep) for d in dims])
    assert 0.97 <= worst <= 0.98 and pm.POOL_MATRIX_P_ULPS == 4 * 0.975, worst

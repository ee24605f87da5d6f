"""-m gpu: the sampled-surface loss (ops.SurfaceLoss) against FLOAT64 on the routes of its backward that no other test holds to
an independent reference -- helpers.fp64_surface_gradient + helpers.rows_close at the bound of tests/test_ops_parity_gpu.py
(ROW_RTOL_SURFACE of an element's term mass + ROW_FLOOR_ULPS coordinate ulps through every term; restated below), the loss at
1e-5 relative.  Every case builds its inputs on the host (meshgen), replays the draws through ops.SurfaceLoss.apply and ASSERTS
THE ROUTE it is there for:

  regs_edge / scratch_edge   per = num + n_gt = 8192 / 8193 points per mesh: the two sides of FIN_REG_POINTS (csrc/finalize_body.h;
                             the host picks surface_finalize_kernel<true / false> by `per <= FIN_REG_POINTS`, csrc/surface_gather.hip)
  scratch, scratch_weighted  the stand-alone scratch variant well past the boundary; with per-mesh weights and an upstream gradient != 1
  crowded                    90 % of the samples on three faces: segments of ~180 ids through the rank pass, walked by the gather
                             eight records at a time
  fits_last                  nf + per + 21 == 38 400: the largest ordering launch the 150 KiB limit admits (csrc/surface_gather.hip:
                             ord_lds_limit, order_lds_bytes)
  overflow                   one point more per cloud: the finalize answers GEOM_EUNSUPPORTED, the forward re-issues it without the
                             ordering and the backward is the fp32-atomic scatter (csrc/sample_loss.hip); with per-mesh weights the
                             forward raises
  long_runs                  the role workgroups of the fused, culled scan launch with runs of one face's samples longer than
                             GROUP_LOOKBACK = 64 (csrc/finalize_body.h): the look-back gives up and everything is ranked

The routes are observed from outside: grad_fn.order (ordered gather / fallback) and the entry points the package issues
(geom_surface_finalize_w_f32 with its want_order argument and its answer, the backward's entry point).  The two boundary numbers
are restated here from the sources, never taken from the library's answer.

Measured margins (GEOM_MARGIN_LOG, MI355X; LAB_NOTES.md section 25), worst element as a share of its bound, one-sided / two-sided:
  regs_edge 0.019 / 0.039    scratch_edge 0.019 / 0.034    scratch 0.015 / 0.028    scratch weighted 0.015
  crowded   0.049 / 0.133    fits_last    0.009 / 0.015    overflow 0.044 / 0.024   long_runs        0.023
(overflow adds in arrival order and moves from run to run: 0.037 / 0.032 in a second run; the others are the same every run;
the fp32 autograd of the reference's expressions sits at 0.05 / 0.20 on the crowded inputs: no route needed a bound of its own).
The float64 side costs 0.1-0.3 s per case and loss (2.5-2.9 s at the 38 000-point cases) and is computed once (lru_cache).
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from helpers import fp64_surface_gradient, rows_close
from geometrics_amd import _lib as L
from geometrics_amd import meshgen, ops
import oracle  # noqa: F401  (helpers.fp64_surface_gradient takes its arg-min indices from the C oracle)

pytestmark = pytest.mark.gpu

# the per-row bound of the surface loss: tests/test_ops_parity_gpu.py, where it is derived and its margins are quoted
ROW_RTOL_SURFACE, ROW_FLOOR_ULPS = 5e-6, 1.0
LOSS_RTOL = 1e-5                # the bar of test_ops_parity_gpu.py for every loss
SCALE = 3000.0

FIN_REG_POINTS = 8192           # csrc/finalize_body.h: points per mesh the register variant of the finalize body holds
GROUP_LOOKBACK = 64             # csrc/finalize_body.h: longest run of one face's samples a role looks back over
# csrc/surface_gather.hip: the ordering launch is refused when order_lds_bytes = (nf + 1 + per + 1024 / 64 + 4) * 4 exceeds
# ord_lds_limit = min(150 KiB, the device's LDS per workgroup - 10 KiB): on gfx950 (160 KiB) nf + per + 21 <= 38 400
GFX950_LDS = 160 * 1024
ORDER_LIMIT_INTS = 150 * 1024 // 4

FINALIZE = "geom_surface_finalize_w_f32"
WANT_ORDER_ARG = 20             # position of want_order among geom_surface_finalize_w_f32's arguments (include/geom_hip.h)
GATHER = "geom_surface_gather_w_f32"
SCATTER_ONE_SIDED, SCATTER_TWO_SIDED = "geom_surface_loss_bwd_f32", "geom_sample_chamfer_bwd_f32"

# level, B, num, n_gt
CASES = {"regs_edge": (2, 2, 4096, 4096), "scratch_edge": (2, 2, 4096, 4097), "scratch": (2, 2, 4600, 4600),
         "crowded": (2, 2, 600, 500), "fits_last": (2, 2, 19030, 19029), "overflow": (2, 2, 19100, 19100)}
MESH_WEIGHT = (0.2, 2.0)
UPSTREAM = 0.37


def test_the_restated_constants_are_the_sources():
    """The numbers the route assertions below are made with, read back from the kernel sources (a changed constant moves the
    boundary the cases sit on: the cases have to move with it)."""
    csrc = os.path.join(os.path.dirname(os.path.abspath(ops.__file__)), "csrc")
    with open(os.path.join(csrc, "finalize_body.h")) as f:
        body = f.read()
    assert int(re.search(r"constexpr int FIN_REG_POINTS = (\d+);", body).group(1)) == FIN_REG_POINTS
    assert int(re.search(r"constexpr int GROUP_LOOKBACK = (\d+);", body).group(1)) == GROUP_LOOKBACK
    with open(os.path.join(csrc, "surface_gather.hip")) as f:
        gather = f.read()
    assert "return limit > 150 * 1024 ? 150 * 1024 : limit;" in gather
    assert "return ((size_t)nf + 1 + per + ORD_WAVES + 4) * sizeof(int);" in gather and "constexpr int ORD_THREADS = 1024;" in gather
    assert "if (per <= geom_finalize::FIN_REG_POINTS) {" in gather
    level, b, num, n_gt = CASES["fits_last"]
    assert 320 + num + n_gt + 21 == ORDER_LIMIT_INTS == 38400
    assert CASES["regs_edge"][2] + CASES["regs_edge"][3] == FIN_REG_POINTS == CASES["scratch_edge"][2] + CASES["scratch_edge"][3] - 1


def device_lds_bytes():
    """The most LDS the current device grants one workgroup, as csrc/device_facts.h asks for it (the largest of three attributes
    of hipDeviceGetAttribute; the enumerators are those of hip_runtime_api.h); None when the runtime does not answer."""
    try:
        hip = ctypes.CDLL("libamdhip64.so")
    except OSError:
        return None
    best = None
    for attribute in (74, 75, 10002):       # MaxSharedMemoryPerBlock, SharedMemPerBlockOptin, MaxSharedMemoryPerMultiprocessor
        value = ctypes.c_int(0)
        if hip.hipDeviceGetAttribute(ctypes.byref(value), attribute, torch.cuda.current_device()) == 0:
            best = value.value if best is None else max(best, value.value)
    return best


def lds_boundary_holds():
    """Whether the 38 400 boundary of fits_last / overflow is this device's: ord_lds_limit is 150 KiB from gfx950's 160 KiB of
    LDS per workgroup on.  A gfx950 that reports less is an error, not a reason to look away."""
    lds = device_lds_bytes()
    if torch.cuda.get_device_properties(0).gcnArchName.startswith("gfx950"):
        assert lds is not None and lds >= GFX950_LDS, "a gfx950 that reports %r bytes of LDS per workgroup" % lds
    return lds is not None and lds >= GFX950_LDS


@pytest.fixture
def calls(monkeypatch):
    """Every entry point the package issues from here on with its answer: (name, code), and (name, code, want_order) for the
    finalize.  (_lib.call goes through _lib.status.)"""
    seen, real = [], L.status

    def spy(name, *args, **kwargs):
        code = real(name, *args, **kwargs)
        seen.append((name, code, int(args[WANT_ORDER_ARG])) if name == FINALIZE else (name, code))
        return code

    monkeypatch.setattr(L, "status", spy)
    return seen


def only(seen, *names):
    return [c for c in seen if c[0] in names]


@functools.lru_cache(maxsize=None)
def _inputs(case):
    level, b, num, n_gt = CASES[case]
    V, Fc = meshgen.icosphere(level)
    verts = meshgen.jittered_batch(V, b)
    gt = meshgen.gt_cloud(b, n_gt)
    ch, u, v = meshgen.sampling_draws(verts, Fc, num)
    if case == "crowded":       # 90 % of the samples moved onto faces 0, 1, 2 (host generator, fixed seed)
        move = np.random.default_rng(1105).random((b, num)) < 0.9
        ch = np.where(move, ch % 3, ch)
    return verts, Fc, gt, ch, u, v                      # shared by every test of the case: never written to


@functools.lru_cache(maxsize=None)
def _exact(case, two_sided):
    """(loss, grad, mass, floor) in float64, once per case and loss."""
    return fp64_surface_gradient(*_inputs(case), two_sided=two_sided, scale=SCALE)


@functools.lru_cache(maxsize=None)
def _exact_mesh_losses(case, two_sided):
    """Every mesh's own loss in float64 (the helper on a batch of one): L_m, where the batch's loss is mean_m L_m."""
    verts, Fc, gt, ch, u, v = _inputs(case)
    return tuple(fp64_surface_gradient(verts[m:m + 1], Fc, gt[m:m + 1], ch[m:m + 1], u[m:m + 1], v[m:m + 1], two_sided=two_sided,
                                       scale=SCALE)[0] for m in range(verts.shape[0]))


def to(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def run(case, two_sided, gpu, mesh_weight=None, upstream=None):
    """One forward + backward of the case's draws: (loss tensor's value, grad_verts, whether the backward was the ordered gather)."""
    verts, Fc, gt, ch, u, v = (to(a, gpu) for a in _inputs(case))
    verts.requires_grad_(True)
    loss = ops.SurfaceLoss.apply(verts, Fc, gt, ch, u, v, two_sided, SCALE, None, None, None, None, mesh_weight)[0]
    ordered = loss.grad_fn.order is not None
    (loss if upstream is None else upstream * loss).backward()
    return float(loss.detach()), verts.grad.clone(), ordered


def assert_stand_alone_ordering(seen):
    """One finalize launch that ordered the points (want_order = 1, answered 0), one gather; the register / scratch variant by
    the host's rule `per <= FIN_REG_POINTS`."""
    assert only(seen, FINALIZE) == [(FINALIZE, 0, 1)], seen
    assert only(seen, GATHER, SCATTER_ONE_SIDED, SCATTER_TWO_SIDED) == [(GATHER, 0)], seen


def check(case, two_sided, got_loss, grad, what, factor=None, exact_loss=None):
    """The loss at LOSS_RTOL, the gradient element by element at the project's bound.  factor [B]: the float64 rows, masses
    and floors of mesh m times factor[m] (per-mesh weight * upstream gradient)."""
    loss64, exact, mass, floor = _exact(case, two_sided)
    if factor is not None:
        f = np.asarray(factor, np.float64).reshape(-1, 1, 1)
        exact, mass, floor = exact * f, mass * np.abs(f), floor * np.abs(f)
        loss64 = exact_loss
    print("%s: loss %.9g, float64 %.9g (%.2e relative)" % (what, got_loss, loss64, abs(got_loss - loss64) / abs(loss64)))
    assert abs(got_loss - loss64) <= LOSS_RTOL * abs(loss64), what
    worst = rows_close(grad.cpu().numpy(), exact, mass, ROW_RTOL_SURFACE, what, floor, ROW_FLOOR_ULPS)
    print("%s: worst gradient element at %.3f of its bound" % (what, worst))


SIDES = pytest.mark.parametrize("two_sided", [False, True], ids=["one_sided", "two_sided"])


@SIDES
@pytest.mark.parametrize("case", ["regs_edge", "scratch_edge", "scratch", "crowded", "fits_last"])
def test_ordered_gather_against_float64(gpu, calls, case, two_sided):
    level, b, num, n_gt = CASES[case]
    per, nf = num + n_gt, _inputs(case)[1].shape[0]
    assert nf == 320
    # the variant of the finalize body the host launches (csrc/surface_gather.hip: per <= geom_finalize::FIN_REG_POINTS)
    assert (per <= FIN_REG_POINTS) == (case in ("regs_edge", "crowded"))
    if case == "crowded":
        longest = max(int(np.bincount(row, minlength=nf).max()) for row in _inputs(case)[3])
        print("crowded: longest segment of samples alone", longest)
        assert longest > 64
    boundary = lds_boundary_holds()
    got_loss, grad, ordered = run(case, two_sided, gpu)
    if case != "fits_last" or boundary:
        assert nf + per + 21 <= ORDER_LIMIT_INTS
        assert ordered
        assert_stand_alone_ordering(calls)
    else:
        print("fits_last: this device reports %r bytes of LDS per workgroup, not gfx950's %d: the route is not asserted"
              % (device_lds_bytes(), GFX950_LDS))
    check(case, two_sided, got_loss, grad, "%s %s" % (case, "two-sided" if two_sided else "one-sided"))
    if ordered:                 # the order is a function of the data: a second pass gives the same bits
        again_loss, again, _ = run(case, two_sided, gpu)
        assert again_loss == got_loss and torch.equal(again, grad)


def test_scratch_variant_with_mesh_weights_and_an_upstream_gradient(gpu, calls):
    """loss = sum_m w[m] * (mesh m's share of the loss) = (1 / B) sum_m w[m] L_m; backward of 0.37 * loss: mesh m's rows are
    0.37 * w[m] times the unweighted ones, and so are the masses and floors of their bound."""
    case = "scratch"
    level, b, num, n_gt = CASES[case]
    assert num + n_gt > FIN_REG_POINTS
    w = torch.tensor(MESH_WEIGHT, dtype=torch.float32, device=gpu)
    got_loss, grad, ordered = run(case, False, gpu, mesh_weight=w, upstream=UPSTREAM)
    assert ordered
    assert_stand_alone_ordering(calls)
    w64 = np.asarray(w.cpu().numpy(), np.float64)                    # the fp32 weights the kernel multiplies by
    exact_loss = float((w64 * np.asarray(_exact_mesh_losses(case, False))).sum() / b)
    assert abs(float(np.mean(_exact_mesh_losses(case, False))) - _exact(case, False)[0]) <= 1e-12 * _exact(case, False)[0]
    check(case, False, got_loss, grad, "scratch weighted one-sided", factor=UPSTREAM * w64, exact_loss=exact_loss)
    again_loss, again, _ = run(case, False, gpu, mesh_weight=w, upstream=UPSTREAM)
    assert again_loss == got_loss and torch.equal(again, grad)


@SIDES
def test_lds_overflow_fallback_against_float64(gpu, calls, two_sided):
    """One point per cloud beyond what the ordering launch holds: loss from the re-issued finalize, gradient from the scatter
    kernels (fp32 atomics in arrival order: the same bound, but no two runs need agree bit for bit)."""
    case = "overflow"
    level, b, num, n_gt = CASES[case]
    boundary = lds_boundary_holds()
    got_loss, grad, ordered = run(case, two_sided, gpu)
    if boundary:
        assert 320 + num + n_gt + 21 > ORDER_LIMIT_INTS
        assert not ordered
        assert only(calls, FINALIZE) == [(FINALIZE, L.EUNSUPPORTED, 1), (FINALIZE, 0, 0)], calls
        scatter = [(SCATTER_TWO_SIDED, 0)] * 2 if two_sided else [(SCATTER_ONE_SIDED, 0)]
        assert only(calls, GATHER, SCATTER_ONE_SIDED, SCATTER_TWO_SIDED) == scatter, calls
    else:
        print("overflow: this device reports %r bytes of LDS per workgroup, not gfx950's %d: the route is not asserted"
              % (device_lds_bytes(), GFX950_LDS))
    check(case, two_sided, got_loss, grad, "overflow %s" % ("two-sided" if two_sided else "one-sided"))


def test_lds_overflow_with_mesh_weights_is_refused(gpu, calls):
    if not lds_boundary_holds():
        print("overflow_weighted: not gfx950's LDS size: the ordering may fit here")
    verts, Fc, gt, ch, u, v = (to(a, gpu) for a in _inputs("overflow"))
    verts.requires_grad_(True)
    w = torch.tensor(MESH_WEIGHT, dtype=torch.float32, device=gpu)
    with pytest.raises(RuntimeError, match="per-mesh weights"):
        ops.SurfaceLoss.apply(verts, Fc, gt, ch, u, v, False, SCALE, None, None, None, None, w)
    assert only(calls, FINALIZE) == [(FINALIZE, L.EUNSUPPORTED, 1)], calls
    torch.cuda.synchronize()


def test_role_workgroups_with_runs_beyond_the_look_back(gpu, calls):
    """The finalize roles of the fused, culled scan launch on the 20-FACE icosahedron (level 0), 8 meshes, 2048 samples and
    2048 gt points each: 8 * 32 = 256 query tiles (the fewest that fuse), 64 <= num < 4096 (the sorted draws), ~100 samples per
    face in consecutive ids -- every run is longer than GROUP_LOOKBACK, so the look-back in front of the wait gives up and every
    id takes the ranking pass.  (The smallest shape with such runs: the library does take the sorted route on 20 faces, so the
    42-vertex sphere with one stretched fan was not needed.)  Against float64 on the draws copied to the host, and bit for bit against the same draws replayed
    without the index (stand-alone finalize, register variant)."""
    level, b, num, n_gt = 0, 8, 2048, 2048
    V, Fc = meshgen.icosphere(level)
    assert Fc.shape[0] == 20
    verts_np, gt_np = meshgen.jittered_batch(V, b), meshgen.gt_cloud(b, n_gt)
    verts, faces, gt = to(verts_np, gpu).requires_grad_(True), to(Fc, gpu), to(gt_np, gpu)
    gi = ops.GtIndex(gt)
    ops.manual_seed(2048)
    try:
        d = ops.draw_samples(verts, faces, num, with_points=True, prepare_scan_for=n_gt, gt_index=gi)
        assert isinstance(d[4], ops.ScanPrep) and d[4].sample_index is not None
        choices, u, v, points = d[:4]
        ch = choices.cpu().numpy()
        assert ch.min() >= 0 and ch.max() < 20
        runs = []
        for row in ch:
            ends = np.flatnonzero(np.diff(row) != 0)
            runs.append(int(np.diff(np.concatenate(([-1], ends, [num - 1]))).max()))
        print("long_runs: longest run of one face's consecutive samples per mesh", runs)
        assert max(runs) > GROUP_LOOKBACK
        del calls[:]
        loss = ops.SurfaceLoss.apply(verts, faces, gt, choices, u, v, False, SCALE, points, d[4], None, gi)[0]
        assert loss.grad_fn.order is not None
        assert only(calls, FINALIZE) == [], calls              # ordered inside the scan launch: no finalize launch of its own
        loss.backward()
        assert only(calls, GATHER, SCATTER_ONE_SIDED, SCATTER_TWO_SIDED) == [(GATHER, 0)], calls
        roles = (float(loss.detach()), verts.grad.clone())
        assert not ops.finalize_roles_gave_up()
        loss64, exact, mass, floor = fp64_surface_gradient(verts_np, Fc, gt_np, ch, u.cpu().numpy(), v.cpu().numpy(), two_sided=False,
                                                           scale=SCALE)
        print("long_runs: loss %.9g, float64 %.9g" % (roles[0], loss64))
        assert abs(roles[0] - loss64) <= LOSS_RTOL * abs(loss64)
        worst = rows_close(roles[1].cpu().numpy(), exact, mass, ROW_RTOL_SURFACE, "long_runs one-sided", floor, ROW_FLOOR_ULPS)
        print("long_runs: worst gradient element at %.3f of its bound" % worst)
        for _ in range(2):      # the same draws without the index: the stand-alone launch; and once more for the order's bits
            del calls[:]
            verts.grad = None
            loss = ops.SurfaceLoss.apply(verts, faces, gt, choices, u, v, False, SCALE)[0]
            loss.backward()
            assert only(calls, FINALIZE) == [(FINALIZE, 0, 1)], calls
            assert float(loss.detach()) == roles[0] and torch.equal(verts.grad, roles[1])
    finally:
        ops.manual_seed(0, gpu)

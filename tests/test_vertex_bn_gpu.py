"""The per-vertex BatchNorm1d(verts) + ReLU + residual-average kernels (csrc/vertex_bn.hip: a scalar and a float4 kernel per
direction) held ELEMENT BY ELEMENT to float64 (helpers.vertex_bn64 / rows_close), straight on the C ABI at the shapes where the
launch rule changes kernel or switches lanes off, and through models.VertexBatchNorm.

Every output's bound is BN_ROW_RTOL = (26 + 8) * 2^-24 of ITS OWN term mass (26 = the longest chain of additions in a
reduction: 16 values per thread, 6 shuffle steps, 4 wave partials; 8 = the project's allowance for the products around it);
the eval-mode forward has no reduction: 8 * 2^-24; grad_residual is one add and one product: bit for bit.  The host-side
self-check (no GPU) is the evidence for the bounds: the kernels' formulas evaluated in plain fp32 torch stay under HALF of them
on every case, and every planted fault -- a row left out of the mean, n - 1 for n, a mask without beta, a forgotten second
gradient, a neighbouring shape's n, a neighbour's gamma -- puts some element outside."""
import types

import numpy as np
import pytest
import torch

from helpers import BN_EVAL_RTOL, BN_MAX_KNIFE, BN_ROW_RTOL, bits, log_margin, rows_close, vertex_bn64

NV, EPS, MOMENTUM, SCALE = 7, 1e-5, 0.1, 0.5
THREADS, VEC_ITERS, MAX_VALUES = 256, 4, 4096


def vec_kernel_serves(b, c, ptr_bits=0, extra_ld=0):
    """The launch rule of csrc/vertex_bn.hip (bn_vec_ok) restated: the float4 kernel wants whole column groups, at most one
    group per thread, 16-byte pointers and row pitches, and at most 4 passes of 256 / (c / 4) rows."""
    if c % 4 or c // 4 > THREADS or ptr_bits & 15 or extra_ld & 3:
        return False
    return b <= VEC_ITERS * (THREADS // (c // 4))


# (b, c, the forward kernel the rule picks, layout variant, why the row is here)
TABLE = [
    (4, 36, "vec", None, "c/4 = 9 leaves 4 lanes off"),
    (3, 4, "vec", None, "c/4 = 1, 253 row slots empty"),
    (1, 4, "vec", None, "n = 4"),
    (4, 1024, "vec", None, "c/4 = 256, b at 4 * rows, n = 4096 at the cap"),
    (20, 192, "vec", None, "b exactly 4 * rows, 16 lanes off"),
    (16, 192, "vec", None, "the training shape"),
    (21, 192, "scalar", None, "c % 4 == 0, one row past the vec limit"),
    (7, 5, "scalar", None, "n < 256"),
    (3, 3, "scalar", None, "narrow c"),
    (2, 2047, "scalar", None, "odd c, per-element division"),
    (1, 4096, "scalar", None, "c/4 > 256, n = 4096 at the cap"),
    (16, 192, "scalar", "x_off1", "x handed over one float past a 16-byte boundary"),
    (4, 36, "scalar", "res_ld61", "residual pitch 61"),
    (4, 36, "vec", "res_ld60", "residual as a column slice at pitch 60"),
]
FAMILIES = ("centred", "offset", "tiny_variance")
MODES = ("full", "plain", "no_affine", "no_grad_residual", "no_param_grads", "eval")
MODE_ROWS = (0, 6, 7)          # (4, 36), (21, 192), (7, 5): every mode; the other rows: "full"
ROW_IDS = ["%dx%d%s" % (b, c, "-" + v if v else "") for b, c, _, v, _ in TABLE]


def _layout(variant, c):
    """(ptr_bits of x, residual pitch) of a row's layout variant."""
    return (4 if variant == "x_off1" else 0), {"res_ld61": 61, "res_ld60": 60}.get(variant, c)


def test_the_table_has_both_kernels_and_the_rule_agrees():
    for b, c, kernel, variant, _ in TABLE:
        assert b * c <= MAX_VALUES
        x_bits, res_ld = _layout(variant, c)
        assert vec_kernel_serves(b, c, x_bits, res_ld) == (kernel == "vec"), (b, c, variant)
    assert sum(k == "vec" for _, _, k, _, _ in TABLE) >= 4 and sum(k == "scalar" for _, _, k, _, _ in TABLE) >= 4
    assert vec_kernel_serves(5, 48)      # 48 columns x 5 rows (the icosphere case of the tapped-layer test): the vec kernel


def make_case(row, family):
    """Seeded inputs of a table row: x = per-vertex offset + spread * N(0, 1); gamma ~ U(0.5, 2), beta ~ U(-1, 1), non-trivial
    old running statistics, N(0, 1) residual and upstream gradients."""
    b, c = TABLE[row][:2]
    rng = np.random.default_rng([1907, row, FAMILIES.index(family)])
    offset, spread = {"centred": (np.zeros(NV), 1.0), "offset": (30.0 * rng.standard_normal(NV), 1.0),
                      "tiny_variance": (np.full(NV, 0.05), 1e-3)}[family]
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return types.SimpleNamespace(
        b=b, c=c, row=row, family=family, what="%s %s" % (ROW_IDS[row], family),
        x=f32(offset.reshape(1, NV, 1) + spread * rng.standard_normal((b, NV, c))),
        gamma=f32(rng.uniform(0.5, 2.0, NV)), beta=f32(rng.uniform(-1.0, 1.0, NV)),
        old_mean=f32(0.5 * rng.standard_normal(NV) + offset), old_var=f32(rng.uniform(0.5, 1.5, NV) * spread ** 2),
        res=f32(rng.standard_normal((b, NV, c))), g=f32(rng.standard_normal((b, NV, c))), g2=f32(rng.standard_normal((b, NV, c))))


def mode_flags(mode):
    """What a mode hands the kernels: (training, relu, residual, second gradient, affine parameters)."""
    return types.SimpleNamespace(training=mode != "eval", relu=mode != "plain", res=mode != "plain", g2=mode not in ("plain", "eval"),
                                 affine=mode != "no_affine", grad_res=mode not in ("plain", "no_grad_residual", "eval"),
                                 param_grads=mode not in ("no_affine", "no_param_grads", "eval"), backward=mode != "eval")


def reference(case, mode):
    """(exact, mass, knife) of a case in a mode: helpers.vertex_bn64."""
    f = mode_flags(mode)
    return vertex_bn64(case.x, case.gamma if f.affine else None, case.beta if f.affine else None, EPS, f.relu,
                       case.res if f.res else None, SCALE, case.g if f.backward else None, case.g2 if f.g2 else None,
                       running=None if f.training else (case.old_mean, case.old_var), momentum=MOMENTUM,
                       old_running=(case.old_mean, case.old_var))


FAULTS = ("mean_skips_last_row", "n_minus_1", "mask_without_beta", "second_gradient_dropped", "neighbouring_n", "neighbours_gamma")


def fp32_evaluation(case, mode, knife, fault=None, victim=0):
    """The kernels' formulas in plain fp32 torch on the host (two-pass statistics, as csrc/vertex_bn.hip), optionally with ONE
    planted fault (the per-vertex ones on the vertex `victim`); the upstream gradients carry zeros at the knife edges.  Returns
    {output: numpy array}."""
    f = mode_flags(mode)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    col = lambda v: v.view(1, -1, 1)
    x = t(case.x)
    b, nv, c = x.shape
    n = b * c
    gamma, beta = (t(case.gamma), t(case.beta)) if f.affine else (torch.ones(nv), torch.zeros(nv))
    if fault == "neighbours_gamma":
        gamma = gamma.clone()
        gamma[victim] = gamma[(victim + 1) % nv]
    out = {}
    if f.training:
        mean = (x[:-1] if fault == "mean_skips_last_row" else x).sum(dim=(0, 2)) / n
        q = ((x - col(mean)) ** 2).sum(dim=(0, 2))
        var = q / (n - 1 if fault == "n_minus_1" else n)
        invstd = 1.0 / torch.sqrt(var + EPS)
        unbiased = (q / (n if fault == "n_minus_1" else n - 1)) if n > 1 else var
        out["running_mean"] = (1.0 - MOMENTUM) * t(case.old_mean) + MOMENTUM * mean
        out["running_var"] = (1.0 - MOMENTUM) * t(case.old_var) + MOMENTUM * unbiased
        out["save_mean"], out["save_invstd"], out["var"] = mean, invstd, var
    else:
        mean, invstd = t(case.old_mean), 1.0 / torch.sqrt(t(case.old_var) + EPS)
    xh = (x - col(mean)) * col(invstd)
    y = xh * col(gamma) + col(beta)
    y = torch.relu(y) if f.relu else y
    out["out"] = (t(case.res) + y) * SCALE if f.res else y
    if f.backward:
        keep = t(~knife)
        go, g2 = t(case.g) * keep, t(case.g2) * keep
        if f.g2:
            if fault == "second_gradient_dropped":
                g2 = g2.clone()
                g2[:, victim, :4] = 0.0
            go = go + g2
        if f.res:
            go = go * SCALE
            out["grad_residual"] = go
        if f.relu:
            go = go * ((xh * col(gamma) if fault == "mask_without_beta" else xh * col(gamma) + col(beta)) > 0)
        sum_g, sum_gx = go.sum(dim=(0, 2)), (go * xh).sum(dim=(0, 2))
        out["grad_bias"], out["grad_weight"] = sum_g, sum_gx
        mgx = sum_gx / ((b + 1) * c if fault == "neighbouring_n" else n)
        out["grad_x"] = col(gamma * invstd) * (go - col(sum_g / n) - xh * col(mgx))
    return {k: v.numpy() for k, v in out.items()}


def expected_grad_residual(case, mode, knife):
    """(g + g2) * scale formed in fp32, as the kernels form it."""
    g = case.g * ~knife
    if mode_flags(mode).g2:
        g = g + case.g2 * ~knife
    return g * np.float32(SCALE)


def compare(got, exact, mass, knife, mode, what, strict):
    """Every output `got` holds against float64, element by element: {output: worst element as a share of its bound}.
    strict: helpers.rows_close (asserts, logs the margins); else only the shares."""
    rtol_fwd = BN_ROW_RTOL if mode != "eval" else BN_EVAL_RTOL
    shares = {}
    for name, value in got.items():
        if name == "grad_residual":
            continue
        pick = ~knife if name == "out" else Ellipsis
        a, e, m = (np.asarray(t, np.float64)[pick] for t in (value, exact[name], mass[name]))
        rtol = rtol_fwd if name == "out" else BN_ROW_RTOL
        if strict:
            shares[name] = rows_close(a, e, m, rtol, "vertex_bn %s %s %s" % (what, mode, name))
        else:
            shares[name] = float((np.abs(a - e) / (rtol * m + 1e-30)).max())
    return shares


def runs():
    """(row, family, mode) of every case: all rows in the full mode, the rows of MODE_ROWS in every mode."""
    for row in range(len(TABLE)):
        for family in FAMILIES:
            for mode in (MODES if row in MODE_ROWS else MODES[:1]):
                yield row, family, mode


def test_fp32_host_evaluation_is_inside_the_bounds_and_every_planted_fault_outside():
    worst, worst_knife = {}, 0.0
    for row, family, mode in runs():
        case = make_case(row, family)
        exact, mass, knife = reference(case, mode)
        assert knife.mean() <= BN_MAX_KNIFE, "%s %s: %d of %d elements on the ReLU's kink" % (case.what, mode, knife.sum(), knife.size)
        worst_knife = max(worst_knife, float(knife.mean()))
        got = fp32_evaluation(case, mode, knife)
        for name, share in compare(got, exact, mass, knife, mode, case.what, strict=False).items():
            assert share <= 0.5, "%s %s %s: the fp32 evaluation sits at %.2f of its bound" % (case.what, mode, name, share)
            worst[name] = max(worst.get(name, 0.0), share)
        if "grad_residual" in got:
            np.testing.assert_array_equal(bits(got["grad_residual"]), bits(expected_grad_residual(case, mode, knife)))
        if mode != "full":
            continue
        # the per-vertex faults go where the data can show them: the vertex whose ReLU lets the most elements through
        victim = int((exact["pre"] > 0).sum(axis=(0, 2)).argmax())
        for fault in FAULTS:
            if (fault == "mean_skips_last_row" and case.b == 1) or (fault == "n_minus_1" and case.b * case.c == 1):
                continue
            bad = fp32_evaluation(case, mode, knife, fault, victim)
            shares = compare(bad, exact, mass, knife, mode, case.what, strict=False)
            # (grad_residual is held bit for bit: a second gradient dropped where the ReLU lets nothing through shows only there)
            shares["grad_residual"] = 2.0 * (not np.array_equal(bits(bad["grad_residual"]), bits(expected_grad_residual(case, mode, knife))))
            assert max(shares.values()) > 1.0, "%s: the planted fault %s stays inside every bound (%r)" % (case.what, fault, shares)
    for name, share in sorted(worst.items()):
        log_margin("vertex_bn fp32 host evaluation " + name, share, 0.5)
    log_margin("vertex_bn knife-edge share", worst_knife, BN_MAX_KNIFE)


# ---- on the device, straight on the C ABI ----------------------------------------------------------------------------------
SENTINEL = -123456.0
PAD = 64            # floats on either side of a buffer (a multiple of 4: the 16-byte alignment of the middle is the slot's)


class Slot:
    """n floats in the middle of a larger allocation filled with a sentinel; `off` floats past a 16-byte boundary."""

    def __init__(self, gpu, n, off=0, values=None):
        self.all = torch.full((n + 2 * PAD + 4,), SENTINEL, dtype=torch.float32, device=gpu)
        assert self.all.data_ptr() % 16 == 0
        self.lo, self.n = PAD + off, n
        self.view = self.all[self.lo:self.lo + n]
        assert self.view.data_ptr() % 16 == 4 * off
        if values is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32).reshape(-1)))
        self.ptr = self.view.data_ptr()

    def numpy(self, shape=None):
        a = self.view.cpu().numpy()
        return a if shape is None else a.reshape(shape)

    def surroundings_intact(self):
        a = self.all.cpu().numpy()
        return bool((a[:self.lo] == SENTINEL).all() and (a[self.lo + self.n:] == SENTINEL).all())

    def untouched(self):
        return bool((self.all.cpu().numpy() == SENTINEL).all())


def run_on_device(gpu, case, mode, knife):
    """Forward (+ backward) of a case on the C ABI with the test's own buffers: ({output: numpy}, the output slots)."""
    from geometrics_amd import _lib
    f = mode_flags(mode)
    b, c, n = case.b, case.c, case.b * NV * case.c
    variant = TABLE[case.row][3]
    x_bits, res_ld = _layout(variant, c)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(gpu)
    x = Slot(gpu, n, off=x_bits // 4, values=case.x)
    gamma, beta = (dev(case.gamma), dev(case.beta)) if f.affine else (None, None)
    res = None
    if f.res:
        wide = np.random.default_rng(5).standard_normal((b, NV, res_ld)).astype(np.float32)
        wide[:, :, :c] = case.res
        res = dev(wide)
        assert res.data_ptr() % 16 == 0
    assert vec_kernel_serves(b, c, x_bits, res_ld if f.res else 0) == (TABLE[case.row][2] == "vec")
    slots = {"out": Slot(gpu, n), "save_mean": Slot(gpu, NV), "save_invstd": Slot(gpu, NV),
             "running_mean": Slot(gpu, NV, values=case.old_mean), "running_var": Slot(gpu, NV, values=case.old_var)}
    _lib.call("geom_vertex_bn_fwd_f32", b, NV, c, x.ptr, _lib.ptr(gamma), _lib.ptr(beta), slots["running_mean"].ptr,
              slots["running_var"].ptr, int(f.training), MOMENTUM, EPS, int(f.relu), _lib.ptr(res), res_ld, SCALE,
              slots["out"].ptr, slots["save_mean"].ptr, slots["save_invstd"].ptr)
    if f.backward:
        keep = ~knife
        g, g2 = dev(case.g * keep), (dev(case.g2 * keep) if f.g2 else None)
        slots.update(grad_x=Slot(gpu, n), grad_residual=Slot(gpu, n), grad_weight=Slot(gpu, NV), grad_bias=Slot(gpu, NV))
        _lib.call("geom_vertex_bn_bwd_f32", b, NV, c, x.ptr, g.data_ptr(), _lib.ptr(gamma), _lib.ptr(beta), slots["save_mean"].ptr,
                  slots["save_invstd"].ptr, int(f.relu), int(f.res), SCALE, slots["grad_x"].ptr,
                  slots["grad_residual"].ptr if f.grad_res else None, slots["grad_weight"].ptr if f.param_grads else None,
                  slots["grad_bias"].ptr if f.param_grads else None, _lib.ptr(g2))
    torch.cuda.synchronize()
    written = {"out"} | ({"save_mean", "save_invstd", "running_mean", "running_var"} if f.training else set())
    if f.backward:
        written |= {"grad_x"} | ({"grad_residual"} if f.grad_res else set()) | ({"grad_weight", "grad_bias"} if f.param_grads else set())
    got = {}
    for name, s in slots.items():
        assert s.surroundings_intact(), "%s %s: the kernel wrote outside %s" % (case.what, mode, name)
        if name in written:
            got[name] = s.numpy((b, NV, c) if s.n == n else None)
        elif name in ("running_mean", "running_var"):
            np.testing.assert_array_equal(bits(s.numpy()), bits(case.old_mean if name == "running_mean" else case.old_var))
        else:
            assert s.untouched(), "%s %s: %s was written although it was not asked for" % (case.what, mode, name)
    assert x.surroundings_intact() and np.array_equal(bits(x.numpy()), bits(case.x.reshape(-1)))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("row", range(len(TABLE)), ids=ROW_IDS)
def test_vertex_bn_kernels_element_by_element_against_float64(gpu, row):
    """Every output of geom_vertex_bn_fwd_f32 / _bwd_f32 at a row of TABLE, on the three input families (and, on the rows of
    MODE_ROWS, in every mode), within its bound of float64; nothing written outside the outputs; grad_residual bit for bit."""
    for family in FAMILIES:
        case = make_case(row, family)
        for mode in (MODES if row in MODE_ROWS else MODES[:1]):
            exact, mass, knife = reference(case, mode)
            assert knife.mean() <= BN_MAX_KNIFE
            log_margin("vertex_bn %s %s knife-edge share" % (case.what, mode), float(knife.mean()), BN_MAX_KNIFE)
            got = run_on_device(gpu, case, mode, knife)
            compare(got, exact, mass, knife, mode, case.what, strict=True)
            if "grad_residual" in got:
                np.testing.assert_array_equal(bits(got["grad_residual"]), bits(expected_grad_residual(case, mode, knife)))


@pytest.mark.gpu
@pytest.mark.parametrize("row", [5, 6], ids=["vec", "scalar"])
def test_vertex_bn_kernels_give_the_same_bits_twice(gpu, row):
    case = make_case(row, "offset")
    _, _, knife = reference(case, "full")
    first, second = run_on_device(gpu, case, "full", knife), run_on_device(gpu, case, "full", knife)
    assert sorted(first) == sorted(second) and len(first) == 9
    for name in first:
        np.testing.assert_array_equal(bits(first[name]), bits(second[name]), err_msg=name)


@pytest.mark.gpu
def test_vertex_bn_host_answers_come_before_anything_is_enqueued(gpu):
    from geometrics_amd import _header, _lib
    einval, eunsupported = _header.CONSTANTS["EINVAL"], _lib.EUNSUPPORTED
    b, c = 4, 36
    n = b * NV * c
    buf = {k: Slot(gpu, n) for k in ("x", "out", "res", "g", "grad_x", "grad_res")}
    vec = {k: Slot(gpu, NV) for k in ("w", "b", "rm", "rv", "sm", "si", "gw", "gb")}

    def fwd(b=b, nv=NV, c=c, x=buf["x"].ptr, res=buf["res"].ptr, res_ld=c):
        return _lib.status("geom_vertex_bn_fwd_f32", b, nv, c, x, vec["w"].ptr, vec["b"].ptr, vec["rm"].ptr, vec["rv"].ptr, 1, MOMENTUM,
                           EPS, 1, res, res_ld, SCALE, buf["out"].ptr, vec["sm"].ptr, vec["si"].ptr)

    def bwd(b=b, nv=NV, c=c, x=buf["x"].ptr):
        return _lib.status("geom_vertex_bn_bwd_f32", b, nv, c, x, buf["g"].ptr, vec["w"].ptr, vec["b"].ptr, vec["sm"].ptr, vec["si"].ptr,
                           1, 1, SCALE, buf["grad_x"].ptr, buf["grad_res"].ptr, vec["gw"].ptr, vec["gb"].ptr, None)

    assert fwd(b=1, c=4097) == eunsupported and bwd(b=1, c=4097) == eunsupported
    assert fwd(b=17, c=241) == eunsupported and bwd(b=17, c=241) == eunsupported          # 4097 = 17 * 241
    assert fwd(x=None) == einval and bwd(x=None) == einval
    assert fwd(res_ld=c - 1) == einval
    assert fwd(b=-1) == einval and bwd(c=-1) == einval
    for empty in (dict(b=0), dict(nv=0), dict(c=0)):
        assert fwd(**empty) == 0 and bwd(**empty) == 0
    torch.cuda.synchronize()
    for s in list(buf.values()) + list(vec.values()):
        assert s.untouched()


# ---- through the module ----------------------------------------------------------------------------------------------------
def _module(gpu, nv, seed):
    from geometrics_amd import models
    rng = np.random.default_rng([1908, seed])
    bn = models.VertexBatchNorm(nv, eps=EPS, momentum=MOMENTUM).to(gpu).train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(rng.uniform(0.5, 2.0, nv).astype(np.float32)))
        bn.bias.copy_(torch.from_numpy(rng.uniform(-1.0, 1.0, nv).astype(np.float32)))
        bn.running_mean.copy_(torch.from_numpy((0.5 * rng.standard_normal(nv)).astype(np.float32)))
        bn.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, nv).astype(np.float32)))
    return bn, rng


@pytest.mark.gpu
@pytest.mark.parametrize("b,c", [(7, 5), (16, 192)], ids=["scalar_7x5", "vec_16x192"])
def test_tapped_vertex_batchnorm_against_the_untapped_layer_and_float64(gpu, b, c):
    """tap=True: the two upstream gradients meet inside the backward kernel (grad_out2) -- the scalar backward at 7 x 5, the
    float4 one at 16 x 192 -- bit for bit what the untapped layer makes of their sum, and within the bounds of float64."""
    import copy
    bn, rng = _module(gpu, NV, b)
    twin = copy.deepcopy(bn)
    assert not vec_kernel_serves(7, 5) and vec_kernel_serves(16, 192)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    x, res, ga, gb = (f32(rng.standard_normal((b, NV, c))) for _ in range(4))
    old = (bn.running_mean.cpu().numpy(), bn.running_var.cpu().numpy())
    weight, bias = bn.weight.detach().cpu().numpy(), bn.bias.detach().cpu().numpy()
    exact, mass, knife = vertex_bn64(x, weight, bias, EPS, True, res, SCALE, ga, gb, momentum=MOMENTUM, old_running=old)
    assert knife.mean() <= BN_MAX_KNIFE
    dev = lambda a: torch.from_numpy(f32(a)).to(gpu)
    ga_d, gb_d = dev(ga * ~knife), dev(gb * ~knife)
    x1, r1 = dev(x).requires_grad_(True), dev(res).requires_grad_(True)
    y, y_again = bn(x1, relu=True, residual=r1, scale=SCALE, tap=True)
    assert y.data_ptr() == y_again.data_ptr() and y is not y_again
    ((y * ga_d).sum() + (y_again * gb_d).sum()).backward()
    x2, r2 = dev(x).requires_grad_(True), dev(res).requires_grad_(True)
    z = twin(x2, relu=True, residual=r2, scale=SCALE)
    z.backward(ga_d + gb_d)
    assert torch.equal(y, z) and torch.equal(x1.grad, x2.grad) and torch.equal(r1.grad, r2.grad)
    assert torch.equal(bn.weight.grad, twin.weight.grad) and torch.equal(bn.bias.grad, twin.bias.grad)
    assert torch.equal(bn.running_mean, twin.running_mean) and torch.equal(bn.running_var, twin.running_var)
    got = {"out": y.detach(), "grad_x": x1.grad, "grad_weight": bn.weight.grad, "grad_bias": bn.bias.grad,
           "running_mean": bn.running_mean, "running_var": bn.running_var}
    compare({k: v.cpu().numpy() for k, v in got.items()}, exact, mass, knife, "full", "module tap %dx%d" % (b, c), strict=True)
    np.testing.assert_array_equal(bits(r1.grad.cpu().numpy()), bits((ga * ~knife + gb * ~knife) * np.float32(SCALE)))


@pytest.mark.gpu
def test_vertex_batchnorm_with_an_upstream_gradient_one_float_into_its_storage(gpu):
    """A contiguous upstream gradient that starts 4 bytes past a 16-byte boundary: the forward ran the float4 kernel, the backward
    has to take the scalar one (the rule looks at every pointer) -- same bounds."""
    b, c = 16, 192
    bn, rng = _module(gpu, NV, 3)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    x, res, g = (f32(rng.standard_normal((b, NV, c))) for _ in range(3))
    exact, mass, knife = vertex_bn64(x, bn.weight.detach().cpu().numpy(), bn.bias.detach().cpu().numpy(), EPS, True, res, SCALE, g)
    assert knife.mean() <= BN_MAX_KNIFE
    dev = lambda a: torch.from_numpy(f32(a)).to(gpu)
    x1, r1 = dev(x).requires_grad_(True), dev(res).requires_grad_(True)
    y = bn(x1, relu=True, residual=r1, scale=SCALE)
    storage = torch.zeros(g.size + 4, device=gpu)
    g_d = storage[1:1 + g.size].view(b, NV, c)
    g_d.copy_(dev(g * ~knife))
    assert g_d.is_contiguous() and g_d.data_ptr() % 16 == 4 and x1.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0
    assert vec_kernel_serves(b, c, y.data_ptr() | x1.data_ptr()) and not vec_kernel_serves(b, c, g_d.data_ptr())
    y.backward(g_d)
    got = {"out": y.detach(), "grad_x": x1.grad, "grad_weight": bn.weight.grad, "grad_bias": bn.bias.grad}
    compare({k: v.cpu().numpy() for k, v in got.items()}, exact, mass, knife, "full", "module offset gradient", strict=True)
    np.testing.assert_array_equal(bits(r1.grad.cpu().numpy()), bits((g * ~knife) * np.float32(SCALE)))


@pytest.mark.gpu
@pytest.mark.parametrize("b,c", [(4, 36), (7, 5)], ids=["vec_4x36", "scalar_7x5"])
def test_running_statistics_after_two_training_steps_against_float64(gpu, b, c):
    """running_mean / running_var after two training-mode calls on inputs with different per-vertex means.  The second step's
    bound carries the first's: mass_2 = (1 - m) * mass_1 + m * (this step's share), and |old_1| <= mass_1."""
    bn, rng = _module(gpu, NV, 4 + c)
    old = tuple(t.cpu().numpy().astype(np.float64) for t in (bn.running_mean, bn.running_var))
    carried = tuple(np.abs(t) for t in old)
    for step in range(2):
        x = (3.0 * rng.standard_normal((1, NV, 1)) + (1.0 + step) * rng.standard_normal((b, NV, c))).astype(np.float32)
        exact, mass, _ = vertex_bn64(x, None, None, EPS, False, None, 1.0, None, momentum=MOMENTUM, old_running=old)
        bn(torch.from_numpy(x).to(gpu))
        old = (exact["running_mean"], exact["running_var"])
        carried = ((1 - MOMENTUM) * carried[0] + MOMENTUM * mass["save_mean"],
                   (1 - MOMENTUM) * carried[1] + MOMENTUM * exact["var"] * (b * c / (b * c - 1.0)))
        assert (carried[0] >= mass["running_mean"] * (1 - 1e-12)).all() and (carried[1] >= mass["running_var"] * (1 - 1e-12)).all()
    rows_close(bn.running_mean.cpu().numpy(), old[0], carried[0], BN_ROW_RTOL, "module running_mean after two steps %dx%d" % (b, c))
    rows_close(bn.running_var.cpu().numpy(), old[1], carried[1], BN_ROW_RTOL, "module running_var after two steps %dx%d" % (b, c))
    assert int(bn.state_dict()["num_batches_tracked"]) == 2

"""GPU: tensors handed to _lib.call are checked against the pointee types of include/geom_hip.h and launch exactly what their
raw addresses launch -- one entry point per pointee class, a list of tensors, an argument struct, two devices."""
import ctypes

import pytest
import torch

from geometrics_amd import _lib, deform, layers, meshgen, ops, utils

pytestmark = pytest.mark.gpu

B, POINTS, SENTINEL = 2, 300, -7


@pytest.fixture(scope="module")
def mesh(gpu):
    """The 162-vertex icosphere: positions [B,V,3], faces, the Laplacian's CSR and the deformation block's adjacency."""
    V, Fc = meshgen.icosphere(2)
    faces = torch.from_numpy(Fc).to(gpu)
    info = utils.adj_init(faces)
    return dict(verts=torch.from_numpy(meshgen.jittered_batch(V, B)).to(gpu), faces=faces, nv=V.shape[0],
                lap=layers.adjacency_csr(info["adj_orig"]), csr=layers.adjacency_csr(info["adj"]))


def _cases(mesh, gpu):
    """name -> (entry point, arguments, positions of the outputs, (position, dtype) of the one mistyped tensor, its name)"""
    torch.manual_seed(11)
    f32 = dict(dtype=torch.float32, device=gpu)
    verts, faces, nv, lap = mesh["verts"], mesh["faces"], mesh["nv"], mesh["lap"]
    nf = faces.shape[0]
    x = torch.randn(1000, **f32)
    cin, c = 1, 192      # the split takes any cin >= 1 and c == 192 only
    planes = torch.empty(3 * int(_lib.lib().geom_dense_dx_split_cinpad(cin)) * c, dtype=torch.int16, device=gpu)
    state = torch.tensor([1234, 0, 0, 0], dtype=torch.int64, device=gpu)
    draws = [torch.empty(B, POINTS, dtype=torch.int64, device=gpu), torch.empty(B, POINTS, **f32), torch.empty(B, POINTS, **f32),
             torch.empty(B, POINTS, 3, **f32)]
    return {
        "float": ("geom_sum_f32", [x.numel(), x, 0.5, torch.empty((), **f32)], [3], (1, torch.float64), "x"),
        "float+int64_t": ("geom_face_areas_f32", [B, nv, verts, nf, faces, torch.empty(B, nf, **f32)], [5], (4, torch.int32),
                          "faces"),
        "int": ("geom_laplacian_f32", [B, nv, lap.rowptr, lap.col, lap.inv_deg, verts, 0, torch.empty_like(verts)], [7],
                (3, torch.int64), "col"),
        "uint16_t": ("geom_dense_dx_split_planes_f32", [cin, c, torch.randn(cin, c, **f32), planes], [3], (3, torch.float32),
                     "planes"),
        "uint64_t": ("geom_draw_samples_rng_f32", [B, nv, verts, nf, faces, POINTS, state] + draws, [6, 7, 8, 9, 10],
                     (6, torch.int32), "rng_state"),
    }


def _fill(args, outputs):
    for i in outputs:
        if args[i].dtype == torch.int64 and args[i].numel() == 4:       # the sampler state: the same start for every run
            args[i].copy_(torch.tensor([1234, 0, 0, 0], dtype=torch.int64))
        else:
            args[i].fill_(SENTINEL)


@pytest.mark.parametrize("pointee", ["float", "float+int64_t", "int", "uint16_t", "uint64_t"])
def test_tensors_launch_what_their_addresses_launch_and_a_wrong_dtype_raises(gpu, mesh, pointee):
    name, args, outputs, (bad_at, bad_dtype), bad_name = _cases(mesh, gpu)[pointee]
    _fill(args, outputs)
    _lib.call(name, *args)
    typed = [args[i].clone() for i in outputs]
    _fill(args, outputs)
    _lib.call(name, *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args])
    for i, t in zip(outputs, typed):
        assert torch.equal(args[i], t), (name, i)
        assert not bool((t == SENTINEL).all()), (name, i)          # (the launch wrote it)
    _fill(args, outputs)
    before = [args[i].clone() for i in outputs]
    wrong = list(args)
    wrong[bad_at] = torch.zeros(args[bad_at].shape, dtype=bad_dtype, device=gpu)
    with pytest.raises(RuntimeError, match=r"%s: parameter `%s` \(declared `\w+ \*%s`\) was given a %s" % (name, bad_name, bad_name,
                                                                                                       str(bad_dtype).replace(".", r"\."))):
        _lib.call(name, *wrong)
    torch.cuda.synchronize()
    for i, t in zip(outputs, before):
        assert torch.equal(args[i], t), (name, i)


def test_a_list_of_tensors_is_the_hand_built_pointer_array(gpu):
    torch.manual_seed(12)
    ts = [torch.randn(777, device=gpu) for _ in range(3)]
    out_list, out_array = torch.empty(777, device=gpu), torch.empty(777, device=gpu)
    _lib.call("geom_sum_tensors_f32", 3, ts, 777, out_list)
    _lib.call("geom_sum_tensors_f32", 3, (ctypes.c_void_p * 3)(*[t.data_ptr() for t in ts]), 777, out_array.data_ptr())
    assert torch.equal(out_list, out_array) and torch.equal(out_list, (ts[0] + ts[1]) + ts[2])
    out_list.fill_(SENTINEL)
    with pytest.raises(RuntimeError, match=r"geom_sum_tensors_f32: parameter `tensors` \(declared `float \*\*tensors`\).*float64"):
        _lib.call("geom_sum_tensors_f32", 3, [ts[0], ts[1].double(), ts[2]], 777, out_list)
    with pytest.raises(RuntimeError, match="takes a list of tensors"):
        _lib.call("geom_sum_tensors_f32", 1, ts[0], 777, out_list)
    torch.cuda.synchronize()
    assert bool((out_list == SENTINEL).all())


def test_an_argument_struct_built_from_tensors(gpu, mesh):
    """One forward launch of the deformation block's layer: the struct built by _lib.args against the same struct filled with
    raw addresses; a float64 bn_w is refused before anything is launched."""
    torch.manual_seed(13)
    nv, csr, c = mesh["nv"], mesh["csr"], 192
    s, bias = torch.randn(B, nv, c, device=gpu), torch.randn(c, device=gpu) * 0.1
    gamma, beta = torch.rand(nv, device=gpu) + 0.5, torch.randn(nv, device=gpu) * 0.2
    mean, invstd = torch.empty(nv, device=gpu), torch.empty(nv, device=gpu)
    tail = deform._tail_tables(csr)
    p = _lib.ptr

    def run(bn_w, typed):
        rm, rv, x = torch.zeros(nv, device=gpu), torch.ones(nv, device=gpu), torch.full_like(s, SENTINEL)
        if typed:
            deform.layer_forward(s, bias, csr, bn_w, beta, rm, rv, True, 0.1, 1e-5, True, None, 0.5, None, x, mean, invstd)
        else:
            a = _lib.DeformFwd(B, nv, c, 64, csr.ell_w, p(s), p(bias), p(csr.ell_col), p(csr.ell_val), p(tail[0]), p(tail[1]),
                               p(bn_w), p(beta), p(rm), p(rv), 1, 0.1, 1e-5, 1, None, 0, 0.5, None, p(x), p(mean), p(invstd),
                               None, None, None, None, 0)
            _lib.call("geom_deform_layer_fwd_f32", ctypes.addressof(a))
        return x, rm, rv

    typed, raw = run(gamma, True), run(gamma, False)
    for a, b in zip(typed, raw):
        assert torch.equal(a, b)
    assert not bool((typed[0] == SENTINEL).any())
    with pytest.raises(RuntimeError, match=r"geom_deform_fwd: parameter `bn_w` \(declared `float \*bn_w`\).*float64"):
        run(gamma.double(), True)
    with pytest.raises(RuntimeError, match="parameter `args`.*was given a geom_deform_bwd"):
        _lib.call("geom_deform_layer_fwd_f32", _lib.DeformBwd())


def test_the_wrappers_refuse_what_they_used_to_pass_on(gpu, mesh):
    lap, verts = mesh["lap"], mesh["verts"]
    with pytest.raises(RuntimeError, match=r"geom_laplacian_f32: parameter `rowptr` \(declared `int \*rowptr`\).*int64"):
        ops.Laplacian.apply(verts, lap.rowptr.long(), lap.col, lap.inv_deg)
    with pytest.raises(RuntimeError, match="set_rng_state"):
        ops.set_rng_state(torch.tensor([1, 0, 0, 0], dtype=torch.int64))
    with pytest.raises(RuntimeError, match="set_rng_state"):
        ops.set_rng_state(torch.zeros(4, dtype=torch.int32, device=gpu))
    with pytest.raises(RuntimeError, match="set_rng_state"):
        ops.set_rng_state(torch.zeros(3, dtype=torch.int64, device=gpu))


def test_a_call_lands_on_the_device_of_its_tensors(gpu):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two HIP devices")
    other = torch.device("cuda:1")
    x = torch.arange(1000, dtype=torch.float32, device=other)
    out = torch.zeros((), device=other)
    assert torch.cuda.current_device() == 0
    _lib.call("geom_sum_f32", x.numel(), x, 1.0, out)
    torch.cuda.synchronize(other)
    assert torch.cuda.current_device() == 0 and float(out) == 499500.0
    with pytest.raises(RuntimeError, match=r"geom_sum_f32: parameter `out`.*the call's other tensors are on cuda:1"):
        _lib.call("geom_sum_f32", x.numel(), x, 1.0, torch.zeros((), device=gpu))

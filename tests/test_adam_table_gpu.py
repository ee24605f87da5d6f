"""GPU: optim.FusedAdam's one-launch route (geom_adam_table_step_f32: per-tensor records in a device table, lr in a device
array) against the chunked route (geom_adam_step_f32, up to 64 tensors per launch) bit for bit, against torch.optim.Adam
within the tolerances of test_fused_adam_graph_replays_track_torch_adam, under HIP-graph replay with an lr change, with
two lr groups, and through state_dict() / load_state_dict() in its own and in torch's format."""
import io

import pytest
import torch

from geometrics_amd import optim

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 3, 4, 5, 1023, 1024, 1025, 4099]
RTOL, ATOL = 2e-5, 2e-6          # test_fused_adam_graph_replays_track_torch_adam's


def _lengths(count):
    """`count` tensor lengths from LENGTHS: all nine (several workgroups, both element paths) as far as they go, then a
    few elements each."""
    return [LENGTHS[i] if i < len(LENGTHS) else (1, 3, 4, 5)[i % 4] for i in range(count)]


def _tensors(count, seed=0, misalign=True):
    """Parameters and gradients of _lengths(count).  Parameter 1 (odd indices among the first nine, where there is more than one
    tensor) is a view one float into its storage: 4-byte but not 16-byte aligned, so the kernel takes the scalar path for it."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    params, grads = [], []
    for i, n in enumerate(_lengths(count)):
        off = 1 if misalign and i % 2 == 1 and i < len(LENGTHS) else 0
        p = torch.randn(n + off + 3, device="cuda", generator=gen)[off:off + n]
        assert p.data_ptr() % 16 == 4 * off or n == 0
        params.append(p.requires_grad_(True))
        grads.append(torch.randn(n, device="cuda", generator=gen))
    return params, grads


def _clone(params):
    """Same values, same alignment."""
    out = []
    for p in params:
        off = (p.data_ptr() % 16) // 4
        q = torch.empty(p.numel() + off + 3, device="cuda")[off:off + p.numel()]
        q.copy_(p.detach())
        out.append(q.requires_grad_(True))
    return out


def _set_grads(params, grads, fresh=False):
    for p, g in zip(params, grads):
        p.grad = g.clone() if fresh else g


def _same(a, b):
    assert a.step_count == b.step_count
    assert torch.equal(a.state[:3], b.state[:3])
    assert int(a.state.view(torch.int32)[3:].abs().sum()) == 0          # arrival counters re-armed
    for x, y in zip(a.params + a.exp_avg + a.exp_avg_sq, b.params + b.exp_avg + b.exp_avg_sq):
        assert torch.equal(x.detach(), y.detach())


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("count", [1, 64, 65, 130])
def test_table_route_equals_chunked_route_bit_for_bit(count, grad_scale):
    params, grads = _tensors(count, seed=count)
    if count == 1:
        params, grads = _tensors(9, seed=1)
        params, grads = params[8:], grads[8:]         # one tensor of 4099 elements: five workgroups, vector path and tail
    other = _clone(params)
    a = optim.FusedAdam(params, lr=1e-2, table=True)
    b = optim.FusedAdam(other, lr=1e-2, table=False)
    for step in range(3):
        _set_grads(params, grads, fresh=step == 1)    # the second step's gradients live elsewhere: the table is uploaded again
        _set_grads(other, grads)
        if grad_scale == 1.0:
            a.step(), b.step()
        else:
            a.step(grad_scale=grad_scale), b.step(grad_scale=grad_scale)
    torch.cuda.synchronize()
    assert a.step_count == 3
    _same(a, b)
    assert all(a._stepped) and a._tab is not None and b._tab is None     # each took its route


def test_a_parameter_without_gradient_is_left_untouched_on_the_table_route():
    params, grads = _tensors(70, seed=2)
    other = _clone(params)
    before = [p.detach().clone() for p in params]
    skipped = (0, 5, 8, 69)
    a = optim.FusedAdam(params, lr=1e-2, table=True)
    b = optim.FusedAdam(other, lr=1e-2, table=False)
    for _ in range(3):
        for k, (p, q, g) in enumerate(zip(params, other, grads)):
            p.grad = q.grad = None if k in skipped else g
        a.step(), b.step()
    _same(a, b)
    for k in skipped:
        assert torch.equal(params[k].detach(), before[k]) and not a.exp_avg[k].any() and not a.exp_avg_sq[k].any()
    assert not torch.equal(params[6].detach(), before[6])


def _torch_steps(ref, ref_opt, grads, steps):
    for _ in range(steps):
        for p, g in zip(ref, grads):
            p.grad = g.clone()
        ref_opt.step()


def _close(ours, ref):
    for a, b in zip(ours, ref):
        assert torch.allclose(a.detach(), b.detach(), rtol=RTOL, atol=ATOL)


def test_table_route_tracks_torch_adam():
    params, grads = _tensors(65, seed=3)
    ref = [p.detach().clone().requires_grad_(True) for p in params]
    opt = optim.FusedAdam(params, lr=1e-3, table=True)
    ref_opt = torch.optim.Adam(ref, lr=1e-3)
    for _ in range(10):
        _set_grads(params, grads, fresh=True)
        opt.step()
    assert opt._tab is not None and opt.step_count == 10
    _torch_steps(ref, ref_opt, grads, 10)
    _close(params, ref)


def _capture(opt):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()                      # warm-up step 1 (eager)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()                      # captured, not executed
    return graph


@pytest.mark.parametrize("moved", [False, True])
def test_captured_table_step_replays_and_follows_a_synced_lr(moved):
    """One eager warm-up step, the table route's step() captured, 9 replays = 10 eager chunked steps bit for bit; then an lr
    change: without sync_hyperparameters() the replay keeps the old lr (documented), with it the next replay uses the new one,
    no re-capture.  moved: the gradients live elsewhere at capture time than in the warm-up, so the capture records the
    table's upload too."""
    params, grads = _tensors(65, seed=4)
    other = _clone(params)
    a = optim.FusedAdam(params, lr=1e-2, table=True)
    b = optim.FusedAdam(other, lr=1e-2, table=False)
    _set_grads(params, grads)
    _set_grads(other, grads)
    if moved:
        first = [g.clone() for g in grads]
        _set_grads(params, first)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            a.step()
        torch.cuda.current_stream().wait_stream(side)
        _set_grads(params, grads)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            a.step()
        assert a._tab.captured and len(a._spare_hosts) == optim._SPARES - 1   # the capture took a pinned buffer set aside for it
    else:
        graph = _capture(a)
        assert a._tab.captured and not a._tabs_kept               # same pointers as the warm-up: nothing uploaded
    for _ in range(9):
        graph.replay()
    for _ in range(10):
        b.step()
    torch.cuda.synchronize()
    assert a.step_count == 10
    _same(a, b)
    # a changed lr that nobody synced: the replay still steps with the old one
    a.param_groups[0]["lr"] = 3e-3
    graph.replay()
    b.step()
    _same(a, b)
    # synced: the next replay uses it
    a.sync_hyperparameters()
    graph.replay()
    b.lr = 3e-3
    b.step()
    torch.cuda.synchronize()
    assert a.step_count == 12
    _same(a, b)
    # an eager step with other gradients afterwards must not disturb what the graph reads
    _set_grads(params, [g.clone() for g in grads])
    a.step()
    _set_grads(params, grads)
    graph.replay()
    b.step(), b.step()
    _same(a, b)


def test_two_groups_with_their_own_lr():
    params, grads = _tensors(70, seed=5)
    other = _clone(params)
    lrs = (1e-2, 1e-3)
    split = 33
    ref = [p.detach().double().clone() for p in params]
    groups = lambda ps: [{"params": ps[:split], "lr": lrs[0]}, {"params": ps[split:]}]
    a = optim.FusedAdam(groups(params), lr=lrs[1], table=True)
    b = optim.FusedAdam(groups(other), lr=lrs[1], table=False)      # chunks never span two lr
    assert [g["lr"] for g in a.param_groups] == list(lrs) and a.lr == lrs[0]
    assert [len(g["params"]) for g in a.param_groups] == [split, 70 - split]
    _set_grads(params, grads)
    _set_grads(other, grads)
    steps = 4
    for _ in range(steps):
        a.step(), b.step()
    _same(a, b)
    # float64 restatement of the update, each group with its own lr
    b1, b2, eps = 0.9, 0.999, 1e-8
    for k, (p, g) in enumerate(zip(ref, grads)):
        m, v, g = torch.zeros_like(p), torch.zeros_like(p), g.double()
        for t in range(1, steps + 1):
            m = b1 * m + (1 - b1) * g
            v = b2 * v + (1 - b2) * g * g
            p -= lrs[k >= split] / (1 - b1 ** t) * m / (v.sqrt() / (1 - b2 ** t) ** 0.5 + eps)
        assert torch.allclose(params[k].detach().double(), p, rtol=RTOL, atol=ATOL)
    # groups with different lr: the in-backward step takes one lr and declines
    from geometrics_amd import backward_pass
    with a.in_backward():
        assert backward_pass.switches.optimizer is None
    one = optim.FusedAdam(groups(other), lr=lrs[0])
    with one.in_backward():
        assert backward_pass.switches.optimizer is one
    with pytest.raises(ValueError, match="betas"):
        optim.FusedAdam([{"params": params[:2]}, {"params": params[2:], "betas": (0.8, 0.999)}])
    with pytest.raises(ValueError, match="eps"):
        optim.FusedAdam([{"params": params[:2]}, {"params": params[2:], "eps": 1e-6}])
    with pytest.raises(ValueError, match="weight decay"):
        optim.FusedAdam(params, weight_decay=1e-4)
    with pytest.raises(ValueError, match="amsgrad"):
        optim.FusedAdam(params, amsgrad=True)


def _through_bytes(sd):
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    return torch.load(buf)


@pytest.mark.parametrize("own_step_state", [True, False])
def test_checkpoint_round_trip_continues_bit_for_bit(own_step_state):
    """5 steps, state_dict() through torch.save / torch.load, load_state_dict() into a fresh optimiser over cloned parameters,
    5 more steps on both: every tensor and the state floats equal the uninterrupted run's.  Without 'geom_step_state' the
    beta powers come from the float32 recurrence."""
    params, grads = _tensors(65, seed=6)
    a = optim.FusedAdam(params, lr=1e-2)
    _set_grads(params, grads)
    for _ in range(5):
        a.step()
    sd = _through_bytes(a.state_dict())
    assert sorted(sd["state"]) == list(range(65)) and sd["geom_step_state"][0] == 5.0
    assert sd["state"][3]["step"].dtype == torch.float32 and sd["state"][3]["step"].dim() == 0 and not sd["state"][3]["step"].is_cuda
    if not own_step_state:
        del sd["geom_step_state"]
    other = _clone(params)
    b = optim.FusedAdam(other, lr=5e-1)               # the checkpoint's lr replaces this one, as in torch
    b.load_state_dict(sd)
    assert b.lr == 1e-2
    _same(a, b)
    _set_grads(other, grads)
    for _ in range(5):
        a.step(), b.step()
    assert b.step_count == 10
    _same(a, b)


def test_checkpoints_interchange_with_torch_adam():
    params, grads = _tensors(65, seed=7, misalign=False)
    ref = [p.detach().clone().requires_grad_(True) for p in params]
    ref_opt = torch.optim.Adam(ref, lr=1e-3)
    _torch_steps(ref, ref_opt, grads, 7)
    # torch -> fused
    ours = [p.detach().clone().requires_grad_(True) for p in ref]
    opt = optim.FusedAdam(ours, lr=1.0)
    opt.load_state_dict(_through_bytes(ref_opt.state_dict()))
    assert opt.step_count == 7 and opt.lr == 1e-3
    _set_grads(ours, grads)
    for _ in range(3):
        opt.step()
    _torch_steps(ref, ref_opt, grads, 3)
    _close(ours, ref)
    # fused -> torch
    back = [p.detach().clone().requires_grad_(True) for p in ours]
    back_opt = torch.optim.Adam(back, lr=1.0)
    back_opt.load_state_dict(_through_bytes(opt.state_dict()))
    for _ in range(3):
        opt.step()
    _torch_steps(back, back_opt, grads, 3)
    _close(ours, back)
    # a wrong shape: ValueError, nothing modified
    held = [t.clone() for t in opt.params + opt.exp_avg + opt.exp_avg_sq] + [opt.state.clone()]
    bad = _through_bytes(ref_opt.state_dict())
    bad["state"][8]["exp_avg_sq"] = torch.zeros(4098)
    bad["param_groups"][0]["lr"] = 7.0
    with pytest.raises(ValueError, match="shape"):
        opt.load_state_dict(bad)
    fewer = _through_bytes(ref_opt.state_dict())
    fewer["param_groups"][0]["params"] = fewer["param_groups"][0]["params"][:-1]
    with pytest.raises(ValueError, match="parameters"):
        opt.load_state_dict(fewer)
    uneven = _through_bytes(ref_opt.state_dict())
    uneven["state"][2]["step"] = torch.tensor(3.0)
    with pytest.raises(ValueError, match="one step counter"):
        opt.load_state_dict(uneven)
    now = opt.params + opt.exp_avg + opt.exp_avg_sq + [opt.state]
    assert all(torch.equal(x.detach(), y) for x, y in zip(now, held)) and opt.lr == 1e-3


def test_a_never_stepped_parameter_stays_out_of_the_state_dict():
    params, grads = _tensors(12, seed=8)
    opt = optim.FusedAdam(params, lr=1e-2, table=True)
    for k, (p, g) in enumerate(zip(params, grads)):
        p.grad = None if k == 7 else g
    opt.step()
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [k for k in range(12) if k != 7]
    assert sd["param_groups"][0]["params"] == list(range(12))
    other = optim.FusedAdam(_clone(params), lr=1e-2, table=True)
    other.load_state_dict(_through_bytes(sd))
    assert sorted(other.state_dict()["state"]) == [k for k in range(12) if k != 7]
    # torch agrees on which parameters have state
    ref = [p.detach().clone().requires_grad_(True) for p in params]
    ref_opt = torch.optim.Adam(ref, lr=1e-2)
    for k, (p, g) in enumerate(zip(ref, grads)):
        p.grad = None if k == 7 else g
    ref_opt.step()
    assert sorted(ref_opt.state_dict()["state"]) == sorted(sd["state"])


def test_a_table_of_only_empty_tensors_still_advances_the_state():
    """The C entry itself (FusedAdam leaves empty tensors out): one workgroup runs, touches no tensor and moves the state."""
    from geometrics_amd import _lib
    state = torch.zeros(_lib.ADAM_STATE_WORDS, device="cuda")
    table = torch.zeros(_lib.lib().geom_adam_table_bytes(2, 0) // 8, dtype=torch.int64, device="cuda")   # n = 0, no addresses
    lr = torch.full((1,), 1e-3, device="cuda")
    args = (2, table.data_ptr(), 0, lr.data_ptr(), 0.9, 0.999, 1e-8, 1.0, state.data_ptr())
    _lib.call("geom_adam_table_step_f32", *args, 0)          # advance = 0: the state stays
    assert not state.any()
    _lib.call("geom_adam_table_step_f32", *args, 1)
    _lib.call("geom_adam_table_step_f32", *args, 1)
    want = torch.tensor([2.0, 0.9, 0.999]).mul(torch.tensor([1.0, 0.9, 0.999]))
    assert torch.equal(state[:3].cpu(), want)
    assert int(state.view(torch.int32)[3:].abs().sum()) == 0


def test_table_step_is_bit_reproducible():
    params, grads = _tensors(130, seed=9)
    runs = []
    for _ in range(2):
        ps = _clone(params)
        opt = optim.FusedAdam(ps, lr=1e-2)            # 129 tensors with elements: three chunked launches, so the table route
        _set_grads(ps, grads)
        for _ in range(3):
            opt.step()
        assert opt._tab is not None
        runs.append(opt)
    _same(*runs)

"""CPU: the host side of the one-launch Adam (geom_adam_table_step_f32, optim.FusedAdam's checkpoints, the overlay's opt-in
`optim`): argument rejection without a device, the float32 beta-power recurrence, and the GEOM_OVERLAY_ADAM switch."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from geometrics_amd import _lib, optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_step_rejects_bad_arguments_without_a_gpu():
    L = _lib.lib()
    one = 0x1000                                     # any non-null, 8-byte aligned address: rejected calls never touch it
    args = (.9, .999, 1e-8, 1.0)                     # beta1, beta2, eps, grad_scale
    assert L.geom_adam_table_step_f32(1, None, 1, None, *args, None, 1, None) == -1
    assert L.geom_adam_table_step_f32(1, None, 1, one, *args, one, 1, None) == -1         # no table
    assert L.geom_adam_table_step_f32(1, one, 1, None, *args, one, 1, None) == -1         # no lr array
    assert L.geom_adam_table_step_f32(1, one, 1, one, *args, None, 1, None) == -1         # no state
    assert L.geom_adam_table_step_f32(1, one + 4, 1, one, *args, one, 1, None) == -1      # table not 8-byte aligned
    assert L.geom_adam_table_step_f32(-1, one, 1, one, *args, one, 1, None) == -1
    assert L.geom_adam_table_step_f32(1, one, -1, one, *args, one, 1, None) == -1
    assert L.geom_adam_table_step_f32(1, one, 0x40000000, one, *args, one, 1, None) == -2  # more workgroups than a launch takes
    assert L.geom_adam_table_step_f32(0, None, 0, None, *args, None, 1, None) == 0        # nothing to do: no launch


def test_table_bytes():
    L = _lib.lib()
    assert L.geom_adam_table_bytes(0, 0) == 0
    assert L.geom_adam_table_bytes(1, 1) == 48 and L.geom_adam_table_bytes(500, 0x3fffffff) == 48 * 500
    assert L.geom_adam_table_bytes(-1, 0) == -1 and L.geom_adam_table_bytes(1, -1) == -1
    assert L.geom_adam_table_bytes(1, 0x40000000) == -2
    assert L.geom_adam_table_bytes(2 ** 31 - 1, 0) == 48 * (2 ** 31 - 1)                  # 64-bit size


@pytest.mark.parametrize("beta", [0.9, 0.999])
def test_beta_power_is_the_kernels_float32_recurrence(beta):
    b = np.float32(beta)
    want, p = {}, None
    for t in range(1, 200001):
        p = b if t == 1 else np.float32(p * b)
        if t in (1, 2, 10, 1000, 200000):
            want[t] = p
    for t, w in want.items():
        got = optim.beta_power(beta, t)
        assert got.dtype == np.float32 and got.tobytes() == w.tobytes(), (beta, t, got, w)
    assert optim.beta_power(beta, 0) == 0.0
    # float32 keeps subnormals (the kernels too): from ~1e-42 on, x * beta rounds back to x and the chain stays there for good
    assert 0.0 < want[200000] < 1e-41 and np.float32(want[200000] * b) == want[200000]
    assert optim.beta_power(beta, 10 ** 12).tobytes() == want[200000].tobytes()           # ... which ends the loop at once


def test_beta_power_is_exact_zero_once_the_chain_has_underflowed():
    """A beta below 0.5 rounds the smallest subnormal down to 0 (0.25 ^ t leaves float32 at t = 75)."""
    b, p = np.float32(0.25), np.float32(0.25)
    for _ in range(99):
        p = np.float32(p * b)
    assert p == 0.0
    assert optim.beta_power(0.25, 74) > 0.0
    for t in (75, 100, 10 ** 12):
        assert optim.beta_power(0.25, t).tobytes() == np.float32(0).tobytes()


def test_beta_power_differs_from_the_closed_form():
    """Why load_state_dict() may not use b ** t: at t = 1000 the float32 chain for 0.999 is not the rounded power."""
    chain = optim.beta_power(0.999, 1000)
    assert chain != np.float32(np.float64(np.float32(0.999)) ** 1000)


def _overlay_probe(tmp_path, value):
    (tmp_path / "utils.py").write_text("import torch.optim as optim\n")
    code = ("import sys, torch, utils\n"
            "assert utils.__file__.startswith(%r), utils.__file__\n"
            "import geometrics_amd.optim as go\n"
            "a = utils.optim.Adam\n"
            "print('ADAM', 'torch' if a is torch.optim.Adam else 'other')\n"
            "print('SGD', utils.optim.SGD is torch.optim.SGD, utils.optim.lr_scheduler is torch.optim.lr_scheduler)\n"
            "try:\n"
            "    a([torch.zeros(3, requires_grad=True)], lr=1e-2, weight_decay=1e-4)\n"
            "    print('BUILT')\n"
            "except ValueError as e:\n"
            "    print('VALUEERROR', e)\n"
            "try:\n"
            "    a([torch.zeros(3, requires_grad=True)], lr=1e-2)\n"
            "    print('BUILT')\n"
            "except RuntimeError as e:\n"
            "    print('RUNTIMEERROR', e)\n" % os.path.join(ROOT, "overlay"))
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1",
               PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "overlay"), ROOT, str(tmp_path)]))
    env.pop("GEOM_OVERLAY_ADAM", None)
    if value is not None:
        env["GEOM_OVERLAY_ADAM"] = value
    other = tmp_path / "cwd"
    other.mkdir(exist_ok=True)
    return subprocess.run([sys.executable, "-c", code], env=env, cwd=str(other), capture_output=True, text=True, timeout=300)


def test_overlay_hands_over_torch_optim_by_default(tmp_path):
    out = _overlay_probe(tmp_path, None)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert lines[0] == "ADAM torch" and lines[1] == "SGD True True"
    assert lines[2] == "BUILT" and lines[3] == "BUILT"            # torch's own Adam: CPU tensors and weight decay are fine


def test_overlay_hands_over_the_fused_adam_on_request(tmp_path):
    out = _overlay_probe(tmp_path, "fused")
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert lines[0] == "ADAM other" and lines[1] == "SGD True True"
    assert lines[2].startswith("VALUEERROR") and "weight decay" in lines[2]      # FusedAdam's constructor: what it does not implement
    assert lines[3].startswith("RUNTIMEERROR") and "HIP device" in lines[3]      # ... and it has no CPU path
    bad = _overlay_probe(tmp_path, "yes")
    assert bad.returncode != 0 and "GEOM_OVERLAY_ADAM" in bad.stderr

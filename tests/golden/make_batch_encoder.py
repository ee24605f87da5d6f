"""Generate tests/golden/batch_mesh_encoder.npz: the reference's BatchMeshEncoder(50) (models.py:386-435) and the latent loss
of its training step (GEOMetrics.py:165-171) in FLOAT64, with the same run in float32 beside it.

    python tests/golden/make_batch_encoder.py

`import make_golden` provides the stubs the reference's modules need, the reference's path and save(); its __main__ guard keeps
it from writing anything.  Per case:

  * parameters: helpers.fill_parameters(enc, seed, gain=6.0) -- the reference initialiser's scale.  At the default gain of 2
    the features nearly collapse and the top-2 gap of the head's max over the vertices is ~1e-7 of scale: float32 then flips
    arg-maxes against float64 and the position gradient moves by 10 % -- a fixture that compares nothing;
  * positions: template + 0.03 * default_rng([seed, 0]).standard_normal, rounded to fp32;
  * adj: the reference's utils.adj_init(faces)["adj"];
  * v [B,V,50]: the `reduce` layer's values before its max (caught where the layer hands them to its activation);
  * target = lat64 + 0.5 * rms(lat64) * seeded_input([seed, 1]), rounded to fp32; on_latent as listed;
  * G = seeded_input([seed, 2], v.shape): a dense cotangent for v.

Asserted and stored: (a) the smallest top-2 gap of v over (mesh, channel) >= 1e-4 of max|v|; (b) min |lat - target| >= 1e-3 of
max|lat| (the L1 kink); (c) every ELU layer's share of negative outputs in [0.05, 0.95]; (d) the reference's float32 v within
5e-6 of scale of its float64 v.  Stored besides: float64 latents, arg-max vertices and gaps, a weighted checksum and 24 sampled
rows of v, the loss, the positions' gradients of the latent loss and of sum(v * G), the float32 run's distance from each of
these (of scale), the gradients of sum(v * G) with respect to h1.weight, h24.weight and 64 sampled rows of reduce.weight_Ws.0,
and the reference's state_dict keys with their shapes."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (stubs, reference path, save())

sys.path.insert(0, os.path.join(make_golden.ROOT, "tests"))
import helpers  # noqa: E402

# case -> (mesh, batch, seed, on_latent)
CASES = {"ico162_b2": ("icosphere_2", 2, 2120, (1.0, 1.0)),
         "uv482_b3": ("uv_sphere", 3, 2106, (1.0, 0.0, 1.0))}
LATENT = 50
WEIGHT = .0005
ROWS = 24
W_ROWS = 64
LAYERS = ("h1", "h21", "h22", "h23", "h24", "h3", "h4", "h41", "h5", "h6", "h7", "h8", "h81", "h9", "h10", "h11")
PARAM_GRADS = ("h1.weight", "h24.weight", "reduce.weight_Ws.0")


def _of_scale(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def mesh_of(name):
    return make_golden.meshgen.uv_sphere() if name == "uv_sphere" else make_golden.meshgen.icosphere(2)


def case_inputs(mesh, batch, seed):
    """(positions [B,V,3] fp32, faces) of a case."""
    V, Fc = mesh_of(mesh)
    noise = np.random.default_rng([seed, 0]).standard_normal((batch,) + V.shape)
    return (V[None].astype(np.float64) + 0.03 * noise).astype(np.float32), Fc


def run(ref_models, dtype, pos, adj, seed, on, target=None):
    """One evaluation of the reference encoder in `dtype`: dict of float64 numpy results (+ `target`, made from the float64
    latents when not given)."""
    import torch.nn.functional as F
    enc = helpers.fill_parameters(ref_models.BatchMeshEncoder(LATENT), seed, gain=6.0).to(dtype)
    caught, shares = {}, []

    def catch(v):
        caught["v"] = v
        return F.elu(v)
    enc.reduce.register_forward_pre_hook(lambda mod, args: (args[0], args[1], catch))
    for name in LAYERS:
        getattr(enc, name).register_forward_hook(lambda mod, args, out: shares.append(float((out < 0).double().mean())))
    p = torch.from_numpy(pos).to(dtype).requires_grad_(True)
    lat = enc(p, adj.to(dtype))
    v = caught["v"]
    out = {"latents": lat.detach().double().numpy(), "v": v.detach().double().numpy(), "negative_share": np.array(shares)}
    if target is None:
        lat64 = out["latents"]
        target = (lat64 + 0.5 * np.sqrt((lat64 ** 2).mean()) * helpers.seeded_input([seed, 1], lat64.shape)).astype(np.float32)
    out["target"] = target
    on_t = torch.tensor(on, dtype=dtype)
    loss = WEIGHT * (torch.mean(torch.abs(lat - torch.from_numpy(target).to(dtype)), dim=1) * on_t / (on_t.sum())).sum()   # GEOMetrics.py:167
    out["loss"] = float(loss.detach().double())
    out["grad_latent_loss"] = torch.autograd.grad(loss, p, retain_graph=True)[0].double().numpy()
    G = torch.from_numpy(helpers.seeded_input([seed, 2], tuple(v.shape))).to(dtype)
    params = dict(enc.named_parameters())
    grads = torch.autograd.grad((v * G).sum(), [p] + [params[k] for k in PARAM_GRADS])
    out["grad_vG"] = grads[0].double().numpy()
    for k, g in zip(PARAM_GRADS, grads[1:]):
        out["grad." + k] = g.double().numpy()
    out["state"] = [(k, tuple(t.shape)) for k, t in enc.state_dict().items()]
    return out


def make_case(ref_models, case, mesh, batch, seed, on):
    pos, Fc = case_inputs(mesh, batch, seed)
    adj = make_golden.ref_utils.adj_init(make_golden.t(Fc))["adj"]
    r64 = run(ref_models, torch.float64, pos, adj, seed, on)
    r32 = run(ref_models, torch.float32, pos, adj, seed, on, target=r64["target"])
    v, lat = r64["v"], r64["latents"]
    nv = v.shape[1]
    top = np.sort(v, axis=1)
    gaps = top[:, -1] - top[:, -2]                                  # [B, latent]
    gap = float(gaps.min() / np.abs(v).max())
    assert gap >= 1e-4, "%s: top-2 gap %.2e of scale" % (case, gap)
    kink = float(np.abs(lat - r64["target"]).min() / np.abs(lat).max())
    assert kink >= 1e-3, "%s: |lat - target| comes within %.2e of scale of the L1 kink" % (case, kink)
    shares = r64["negative_share"]
    assert ((shares >= 0.05) & (shares <= 0.95)).all(), "%s: negative shares %s" % (case, shares)
    spread = {k: _of_scale(r32[k], r64[k]) for k in ("v", "latents", "grad_latent_loss", "grad_vG")}
    spread["loss"] = abs(r32["loss"] - r64["loss"]) / abs(r64["loss"])
    assert spread["v"] <= 5e-6, "%s: float32 v is %.2e of scale from float64" % (case, spread["v"])
    assert (np.argmax(r32["v"], axis=1) == np.argmax(v, axis=1)).all()
    rng = np.random.default_rng([seed, 7])
    rows_v = rng.choice(nv, ROWS, replace=False).astype(np.int32)
    rows_v[0], rows_v[1] = 0, nv - 1                                 # (the uv sphere's two pole rows)
    rows_b = rng.integers(0, batch, ROWS).astype(np.int32)
    w_rows = np.sort(rng.choice(300, W_ROWS, replace=False)).astype(np.int32)
    out = dict(mesh=np.array(mesh), batch=np.int64(batch), nv=np.int64(nv), seed=np.int64(seed), on_latent=np.array(on, np.float32),
               weight=np.float64(WEIGHT), in_ck=np.float64(pos.astype(np.float64).sum()), target=r64["target"],
               latents=lat, argmax=np.argmax(v, axis=1).astype(np.int32), gaps=gaps, min_gap=np.float64(gap), kink=np.float64(kink),
               negative_share=shares, v_ck=helpers.weighted_checksum("v", v), rows_b=rows_b, rows_v=rows_v,
               v_rows=v[rows_b, rows_v].astype(np.float32), v_scale=np.float64(np.abs(v).max()), loss=np.float64(r64["loss"]),
               grad_latent_loss=r64["grad_latent_loss"].astype(np.float32), grad_vG=r64["grad_vG"].astype(np.float32),
               w_rows=w_rows)
    out.update({"float32." + k: np.float64(s) for k, s in spread.items()})
    for k in PARAM_GRADS:
        g = r64["grad." + k]
        out["grad." + k] = (g[w_rows] if k.startswith("reduce") else g).astype(np.float32)
    print("%-10s gap %.1e kink %.1e shares %.2f..%.2f float32: %s" % (case, gap, kink, shares.min(), shares.max(),
                                                                      " ".join("%s %.1e" % kv for kv in spread.items())))
    return out, r64["state"]


def make_batch_encoder():
    import models as ref_models                      # the reference's models.py
    assert ref_models.__file__.startswith(make_golden.REF)
    arrays = {}
    for case, (mesh, batch, seed, on) in CASES.items():
        out, state = make_case(ref_models, case, mesh, batch, seed, on)
        arrays.update({"%s.%s" % (case, k): v for k, v in out.items()})
    arrays["state_keys"] = np.array([k for k, _ in state])
    arrays["state_shapes"] = np.array([list(s) + [0] * (2 - len(s)) for _, s in state], np.int32)
    make_golden.save("batch_mesh_encoder", **arrays)


if __name__ == "__main__":
    make_batch_encoder()

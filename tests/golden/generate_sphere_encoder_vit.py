#!/usr/bin/env python3
"""Golden vectors of the ViT Sphere Encoder (runs ONLY in the build container, on the CPU, never on the GPU box).

Imports the reference's models package by path like generate_sphere_encoder.py, whose recorder and seed search this reuses, and
records from the reference's own class SphereEncoderViT with use_perceptual=False, for two tiny networks, the same record set: the
initial state_dict (sd0.*), the working state every later record starts from (sdw.*: the initial one with head_dec.weight scaled by
HEAD_GAIN, so that pix_con reaches the linear smooth-L1 branch), the input, every torch.rand / torch.randn draw of the forward in order (and assembled as u [B, 4] and e [B, L]),
every forward output, the loss dict, the per-loss gradient of every parameter by plain autograd, the summed gradient, the state after
one Adam(1e-3) step, a second step's losses, an eval-mode forward and its losses, and sample(2, steps=3, share_noise=True) with its e.

Case 1: N = 16 tokens (one full 16-key tile), head_dim 16.  Case 2 (mix): N = 25 (a ragged second tile), head_dim 6 (padded to 8), the
mixed-angle schedule and non-default lambdas.

Usage:  python tests/golden/generate_sphere_encoder_vit.py        (seconds)
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("MOVAE_REFERENCE", "/root/reference")

#: (tag, first seed tried, B, constructor keywords)
CASES = [
    ("sphere_encoder_vit_tiny", 3, 3,
     dict(img_size=8, patch_size=2, embed_dim=16, depth=2, num_heads=1, mixer_depth=1, mixer_tokens_mlp_dim=8, mixer_channels_mlp_dim=32,
          latent_channels=4)),  # (embed_dim 32 / two heads makes a fixture of 1.8 MB; the kernel tests cover several heads at head_dim 16)
    ("sphere_encoder_vit_tiny_mix", 3, 3,
     dict(img_size=10, patch_size=2, embed_dim=12, depth=2, num_heads=2, mixer_depth=1, mixer_tokens_mlp_dim=8, mixer_channels_mlp_dim=24,
          latent_channels=4, sigma_mix_prob=0.5, sigma_mix_angle_min_deg=80.0, sigma_mix_angle_max_deg=85.0, lambda_pix_recon=0.8,
          lambda_pix_con=0.3, lambda_lat_con=0.2, pix_recon_smooth_l1_weight=0.9, pix_con_smooth_l1_weight=0.4)),
]


#: factor on head_dec.weight between the initial state (sd0.*) and the working state (sdw.*) every other record starts from
HEAD_GAIN = 6.0


def _load(name):
    spec = importlib.util.spec_from_file_location("_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _attempt(gg, gs, seed, B, kw):
    """One recording at `seed`: (fixture dict, None) or (None, why the assertions fail)."""
    from models.sphere_encoder_vit import SphereEncoderViT

    _np, _Draws = gg._np, gs._Draws
    out = {}
    torch.manual_seed(seed)
    np.random.seed(seed)
    net = SphereEncoderViT(use_perceptual=False, device=torch.device("cpu"), **kw)
    net.train()
    for k, v in net.state_dict().items():
        out[f"sd0.{k}"] = _np(v)
    # The working state: at its initial weights the decoder's two outputs never differ by 1, so pix_con would stay on the quadratic
    # smooth-L1 branch.  The head's weight is scaled up (its output saturates the tanh) and everything below starts from this state.
    with torch.no_grad():
        net.head_dec.weight.mul_(HEAD_GAIN)
    for k, v in net.state_dict().items():
        out[f"sdw.{k}"] = _np(v)
    size = kw["img_size"]
    # inputs in [-1, 1], the range of the tanh output: the random-weight decoder's output then differs from the input by more than 1 somewhere
    x = torch.rand(B, 3, size, size, generator=torch.Generator().manual_seed(seed + 1)) * 2.6 - 1.3
    out["x"] = _np(x)
    out["meta"] = np.array([f"seed={seed}", f"B={B}", f"head_gain={HEAD_GAIN}", f"kwargs={kw!r}"])
    out["objectives"] = np.array(list(net.objectives.keys()))
    with _Draws() as rec:
        outputs = net(x)
    mix = kw.get("sigma_mix_prob", 0.0) > 0
    kinds = [k for k, _ in rec.draws]
    assert kinds == (["rand", "rand", "rand", "rand", "randn"] if mix else ["rand", "rand", "randn"]), kinds
    for i, (k, t) in enumerate(rec.draws):
        out[f"draw.{i}.{k}"] = _np(t)
    d = [t for _, t in rec.draws]
    zero = torch.zeros(B, 1)
    out["u"] = _np(torch.cat([d[0], d[1], d[2], d[3]] if mix else [d[0], zero, zero, d[1]], dim=1))
    out["e"] = _np(d[-1])
    if mix:
        taken = d[1] < kw["sigma_mix_prob"]
        if not (taken.any() and (~taken).any()):
            return None, "the mix band takes all rows or none"
    loss_dict = net.loss_function(x, args=outputs)
    for name, a, b in (("pix_recon", outputs["recons"], x), ("pix_con", outputs["x_recon_NOISY"], outputs["x_recon_noisy_small_sg"])):
        frac = ((a - b).abs() >= 1).float().mean().item()
        if not gs.MIN_FRACTION <= frac <= 1 - gs.MIN_FRACTION:
            return None, f"{name}: {frac:.3%} of the elements on the linear smooth-L1 branch"
        out[f"linear_fraction.{name}"] = np.array(frac)
    for k, v in outputs.items():
        out[f"out.{k}"] = _np(v)
    for k, v in loss_dict.items():
        out[f"loss.{k}"] = _np(v)
    names = [n for n, _ in net.named_parameters()]
    params = [p for _, p in net.named_parameters()]
    comp = [(k, v) for k, v in loss_dict.items() if k != "total_loss"]
    for i, (k, v) in enumerate(comp):
        gs_ = torch.autograd.grad(v, params, retain_graph=True, allow_unused=True)
        assert all(g is not None for g in gs_), f"{k} leaves a parameter without a gradient"
        for n, g in zip(names, gs_):
            out[f"gloss.{i}.{n}"] = _np(g)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    opt.zero_grad()
    loss_dict["total_loss"].backward()
    for n, p in zip(names, params):
        out[f"gsum.{n}"] = _np(p.grad)
    opt.step()
    for k, v in net.state_dict().items():
        out[f"sd1.{k}"] = _np(v)
    with _Draws(rec.draws):
        outputs2 = net(x)
    for k, v in net.loss_function(x, args=outputs2).items():
        out[f"loss2.{k}"] = _np(v)
    net.eval()
    with torch.no_grad(), _Draws(rec.draws):
        oe = net(x)
        le = net.loss_function(x, args=oe)
    for k, v in oe.items():
        out[f"eval.{k}"] = _np(v)
    for k, v in le.items():
        out[f"eval_loss.{k}"] = _np(v)
    with _Draws() as srec:
        xs = net.sample(2, device=torch.device("cpu"), steps=3, share_noise=True)
    assert [k for k, _ in srec.draws] == ["randn"]
    out["sample.e"], out["sample.x"] = _np(srec.draws[0][1]), _np(xs)
    return out, None


def model_fixture(gg, gs, tag, seed0, B, kw):
    for seed in range(seed0, seed0 + 256):
        out, why = _attempt(gg, gs, seed, B, kw)
        if out is not None:
            break
        print(f"{tag}: seed {seed} rejected ({why})")
    else:
        raise AssertionError(f"{tag}: no seed in [{seed0}, {seed0 + 256}) satisfies the assertions")
    path = os.path.join(HERE, f"{tag}.npz")
    np.savez_compressed(path, **out)
    print(f"{tag}.npz seed={seed} keys={len(out)} bytes={os.path.getsize(path)} linear fractions: "
          f"{float(out['linear_fraction.pix_recon']):.3f} {float(out['linear_fraction.pix_con']):.3f}")


if __name__ == "__main__":
    gg, gs = _load("generate_golden"), _load("generate_sphere_encoder")
    gg._install_placeholders()
    sys.path.insert(0, REF)
    torch.set_num_threads(8)
    for c in CASES:
        model_fixture(gg, gs, *c)

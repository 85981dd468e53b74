#!/usr/bin/env python3
"""Step time of a reduced ViT Sphere Encoder at the CIFAR shape (32 x 32, patch 2: N = 256 tokens; embed 256, depth 4, heads 8, mixer
depth 2, batch 64, UPGrad, fp32) and the time of the new kernel pairs against the torch composition of the reference's expressions.

Times the eager step (train.train_step) and the captured step (train.GraphedTrainStep replay, noise drawn in the kernel), and
forward + backward of: the attention with RoPE on the packed projection at B * heads x N x hd for hd = 32 and 64, LayerNorm and RMSNorm
on [B * N, embed], bias + GELU on [B * N, 4 * embed] -- each against the same expression in torch on the same device and operands
(median of --repeats windows, alternating the two).  The default 24 x 1024 model of the reference is a 600 M-parameter network and is
not what this measures.  Prints one JSON line.  bench.py's fixed configurations are not touched.

Usage:  python tools/vit_sphere_bench.py [--steps 20] [--warmup 5] [--repeats 7] [--dtype fp32|bf16]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Args:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--embed", type=int, default=256)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--mixer_depth", type=int, default=2)
    ap.add_argument("--agg", default="upgrad")
    ap.add_argument("--skip_model", action="store_true")
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="fp32",
                    help="compute dtype of the model steps and the attention rows (movae_set_compute_dtype); the torch side stays fp32")
    a = ap.parse_args()

    import torch
    import torch.nn.functional as F

    import movae_amd  # noqa: F401
    from movae_amd import _lib as L
    from movae_amd import aggregation, ops
    from movae_amd.models import build_sphere_encoder_vit
    from movae_amd.train import GraphedTrainStep, make_optimizer, train_step

    dev = torch.device("cuda:0")
    L.set_compute_dtype(a.dtype)
    B, N = a.batch, 256
    args = Args(latent_dim=N * 8, vit_embed_dim=a.embed, vit_depth=a.depth, vit_num_heads=a.heads, vit_mixer_depth=a.mixer_depth,
                aggregator=a.agg, agg_norm_eps=1e-4, agg_reg_eps=1e-4, mgda_epsilon=1e-5, mgda_max_iters=250, pref_weights=None,
                optimizer="adam", lr=1e-4, wd=0, momentum=0.9, max_grad_norm=None)
    x = (torch.rand(B, 3, 32, 32, generator=torch.Generator().manual_seed(0)) * 2 - 1).to(dev)
    res = {"arch": "sphere_encoder_vit", "batch": B, "agg": a.agg, "dtype": a.dtype,
           "shape": f"CIFAR (32x32, patch 2, N {N}, embed {a.embed}, depth {a.depth}, heads {a.heads}, mixer depth {a.mixer_depth}, {a.dtype})"}

    def fresh():
        torch.manual_seed(0)
        net = build_sphere_encoder_vit(32, 3, args, dev).to(dev).train()
        return net, make_optimizer(net, args, capturable=True), aggregation.make_aggregator(args)

    if not a.skip_model:
        net, opt, agg = fresh()
        res["parameters"] = sum(p.numel() for p in net.parameters())
        for _ in range(a.warmup):
            train_step(net, x, opt, agg, args)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            train_step(net, x, opt, agg, args)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / a.steps * 1e3
        res["eager_ms_per_step"], res["eager_images_per_s"] = ms, B / (ms * 1e-3)
        net, opt, agg = fresh()
        gs = GraphedTrainStep(net, opt, agg, args, x, warmup=3)
        for _ in range(a.warmup):
            gs.step(x)
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.steps):
            gs.step(x)
        end.record()
        torch.cuda.synchronize()
        ms = start.elapsed_time(end) / a.steps
        res["graphed_ms_per_step"], res["graphed_images_per_s"] = ms, B / (ms * 1e-3)
        res["finite"] = all(math.isfinite(float(v.item())) for v in gs.loss_dict.values())
        del gs, net, opt

    def window(fn, iters=50):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / iters * 1e3  # us per forward + backward, eager launches

    def versus(name, hip_fn, torch_fn):
        for fn in (hip_fn, torch_fn):
            window(fn, 10)
        th, tt = [], []
        for _ in range(a.repeats):  # alternate the two
            th.append(window(hip_fn))
            tt.append(window(torch_fn))
        res[f"{name}_hip_us"], res[f"{name}_torch_us"] = statistics.median(th), statistics.median(tt)
        res[f"{name}_hip_us_spread"], res[f"{name}_torch_us_spread"] = [min(th), max(th)], [min(tt), max(tt)]

    g = torch.Generator().manual_seed(1)
    for hd in (32, 64):
        heads = a.heads
        C = heads * hd
        qkv = torch.randn(B, N, 3 * C, generator=g).to(dev).requires_grad_(True)
        cot = torch.randn(B, N, C, generator=g).to(dev)
        inv_freq = 1.0 / (10000.0 ** (torch.arange(0, hd, 2).float() / hd))
        cos, sin = ops.rope_tables(N, inv_freq, dev)

        def attn_torch():  # AttentionWithRoPE.forward between its two linears (models/sphere_encoder_vit.py:159-166)
            q, k, v = qkv.reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)

            def rotate(t):
                t1, t2 = t[..., 0::2], t[..., 1::2]
                return torch.stack([t1 * cos - t2 * sin, t1 * sin + t2 * cos], dim=-1).flatten(-2)

            attn = ((rotate(q) @ rotate(k).transpose(-2, -1)) * hd ** -0.5).softmax(dim=-1)
            return torch.autograd.grad((attn @ v).transpose(1, 2).reshape(B, N, C), qkv, cot)[0]

        def attn_hip():
            return torch.autograd.grad(ops.attention(qkv, heads, cos, sin), qkv, cot)[0]

        versus(f"attention_hd{hd}", attn_hip, attn_torch)

    D = a.embed
    xr = torch.randn(B * N, D, generator=g).to(dev).requires_grad_(True)
    w = torch.randn(D, generator=g).to(dev).requires_grad_(True)
    b = torch.randn(D, generator=g).to(dev).requires_grad_(True)
    cot = torch.randn(B * N, D, generator=g).to(dev)
    versus("layernorm", lambda: torch.autograd.grad(ops.layer_norm(xr, w, b), [xr, w, b], cot),
           lambda: torch.autograd.grad(F.layer_norm(xr, (D,), w, b, 1e-5), [xr, w, b], cot))
    versus("rmsnorm", lambda: torch.autograd.grad(ops.rms_norm(xr, w), [xr, w], cot),
           lambda: torch.autograd.grad(xr / (xr.pow(2).mean(dim=-1, keepdim=True) + 1e-6).sqrt() * w, [xr, w], cot))
    xg = torch.randn(B * N, 4 * D, generator=g).to(dev).requires_grad_(True)
    bg = torch.randn(4 * D, generator=g).to(dev).requires_grad_(True)
    cg = torch.randn(B * N, 4 * D, generator=g).to(dev)
    versus("bias_gelu", lambda: torch.autograd.grad(ops.bias_gelu(xg, bg), [xg, bg], cg),
           lambda: torch.autograd.grad(F.gelu(xg + bg), [xg, bg], cg))
    print(json.dumps(res))


if __name__ == "__main__":
    main()

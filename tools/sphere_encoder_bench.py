#!/usr/bin/env python3
"""Step time of the conv Sphere Encoder at the CIFAR shape: batch 256, 32 x 32, hidden 32..512, L = 128, UPGrad, fp32.

Times the eager step (train.train_step) and the captured step (train.GraphedTrainStep replay, noise drawn in the kernel), counts
the kernel nodes of the captured graph -- the launches one replayed step makes -- and times the two fused kernel pairs
(ops.SphereLatents, ops.SphereLosses: forward + backward with all three cotangents / the total's cotangent) against the torch
composition of the reference's own expressions on the same device and operands (median of --repeats windows, alternating the two).
Prints one JSON line.  bench.py's fixed configurations are not touched.

Usage:  python tools/sphere_encoder_bench.py [--steps 30] [--warmup 5] [--repeats 7]
"""
import argparse
import ctypes
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
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--latent", type=int, default=128)
    ap.add_argument("--agg", default="upgrad")
    a = ap.parse_args()

    import torch
    import torch.nn.functional as F

    import movae_amd  # noqa: F401
    from movae_amd import aggregation, ops
    from movae_amd.models import build_sphere_encoder
    from movae_amd.train import GraphedTrainStep, make_optimizer, train_step

    dev = torch.device("cuda:0")
    B, L = a.batch, a.latent
    args = Args(batch_size=B, dataset_size=50000, recons_objective="mse", recons_activation=None, latent_dim=L,
                hidden_dims=[32, 64, 128, 256, 512], aggregator=a.agg, agg_norm_eps=1e-4, agg_reg_eps=1e-4, mgda_epsilon=1e-5,
                mgda_max_iters=250, pref_weights=None, optimizer="adam", lr=1e-3, wd=0, momentum=0.9, max_grad_norm=None)
    x = torch.rand(B, 3, 32, 32, generator=torch.Generator().manual_seed(0)).to(dev)
    res = {"arch": "sphere_encoder", "batch": B, "agg": a.agg, "shape": f"CIFAR (32x32, hidden 32..512, L {L}, fp32)"}

    def fresh():
        torch.manual_seed(0)
        net = build_sphere_encoder(32, 3, args, dev).to(dev).train()
        return net, make_optimizer(net, args, capturable=True), aggregation.make_aggregator(args)

    class KeptGraph(torch.cuda.CUDAGraph):  # keeps the captured graph so that its nodes can be counted
        def __new__(cls, *a, **k):
            return super().__new__(cls, keep_graph=True)

        def __init__(self, *a, **k):
            super().__init__(keep_graph=True)

    def kernel_nodes(graph):
        try:
            hip = ctypes.CDLL("libamdhip64.so")
            g = ctypes.c_void_p(graph.raw_cuda_graph())
            n = ctypes.c_size_t(0)
            assert hip.hipGraphGetNodes(g, None, ctypes.byref(n)) == 0
            nodes = (ctypes.c_void_p * n.value)()
            assert hip.hipGraphGetNodes(g, nodes, ctypes.byref(n)) == 0
            kinds = [ctypes.c_int(-1) for _ in range(n.value)]
            for node, kd in zip(nodes, kinds):
                assert hip.hipGraphNodeGetType(ctypes.c_void_p(node), ctypes.byref(kd)) == 0
            return sum(1 for kd in kinds if kd.value == 0)  # hipGraphNodeTypeKernel
        except Exception as e:  # noqa: BLE001
            return f"unavailable ({type(e).__name__}: {e})"

    # ---- the step: eager, then captured -------------------------------------------------------------------------------------
    net, opt, agg = fresh()
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
    orig, torch.cuda.CUDAGraph = torch.cuda.CUDAGraph, KeptGraph
    try:
        gs = GraphedTrainStep(net, opt, agg, args, x, warmup=3)
    finally:
        torch.cuda.CUDAGraph = orig
    res["graphed_kernels_per_step"] = kernel_nodes(gs.graph)
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

    # ---- the two kernel pairs against the torch composition of the reference's expressions --------------------------------------
    g = torch.Generator().manual_seed(1)
    radius, amax = math.sqrt(L), 80.0
    z = torch.randn(B, L, generator=g).to(dev).requires_grad_(True)
    e, u = torch.randn(B, L, generator=g).to(dev), torch.rand(B, 4, generator=g).to(dev)
    cots = [torch.randn(B, L, generator=g).to(dev) for _ in range(3)]

    def rms_norm(t):
        return t / (t.pow(2).mean(dim=-1, keepdim=True) + 1e-6).sqrt()

    def latents_torch():  # models/sphere_encoder.py:196-220 on given draws
        v = rms_norm(z) * radius
        sigma = torch.tan(u[:, 0:1] * amax * (math.pi / 180.0))
        sigma_sub = (u[:, 3:4] * 0.5) * sigma
        vn = rms_norm(v + sigma * e) * radius
        vs = rms_norm(v + sigma_sub * e) * radius
        return torch.autograd.grad([v, vn, vs], z, cots)[0]

    def latents_hip():
        out = ops.sphere_latents(z, (amax, 0.0, 0.0, 0.0), radius, e=e, u=u)
        return torch.autograd.grad(out[:3], z, cots)[0]

    n_img = (B, 32, 32, 3)
    xi = torch.rand(n_img, generator=g).to(dev)
    r = torch.tanh(torch.randn(n_img, generator=g)).to(dev).requires_grad_(True)
    xn = torch.tanh(torch.randn(n_img, generator=g)).to(dev).requires_grad_(True)
    v = (rms_norm(torch.randn(B, L, generator=g)) * radius).to(dev).requires_grad_(True)
    ve = (rms_norm(torch.randn(B, L, generator=g)) * radius).to(dev).requires_grad_(True)
    lam, w = (1.0, 0.5, 0.1), (1.0, 0.5)

    def losses_torch():  # models/sphere_encoder.py:249-283 without the perceptual term
        rec = lam[0] * (w[0] * F.smooth_l1_loss(r, xi, reduction="mean"))
        con = lam[1] * (w[1] * F.smooth_l1_loss(xn, r.detach(), reduction="mean"))
        lat = lam[2] * (1 - F.cosine_similarity(v, ve, dim=-1)).mean()
        return torch.autograd.grad(rec + con + lat, [r, xn, v, ve])

    def losses_hip():
        return torch.autograd.grad(ops.sphere_losses(r, xi, xn, v, ve, lam, w, sg=r.detach())[3], [r, xn, v, ve])

    def window(fn, iters=200):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / iters * 1e3  # us per forward + backward, eager launches

    for name, hip_fn, torch_fn in (("latents", latents_hip, latents_torch), ("losses", losses_hip, losses_torch)):
        for fn in (hip_fn, torch_fn):
            window(fn, 20)
        th, tt = [], []
        for _ in range(a.repeats):  # alternate the two
            th.append(window(hip_fn))
            tt.append(window(torch_fn))
        res[f"{name}_hip_us"], res[f"{name}_torch_us"] = statistics.median(th), statistics.median(tt)
        res[f"{name}_hip_us_spread"], res[f"{name}_torch_us_spread"] = [min(th), max(th)], [min(tt), max(tt)]
    print(json.dumps(res))


if __name__ == "__main__":
    main()

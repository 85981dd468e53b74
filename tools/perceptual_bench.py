#!/usr/bin/env python3
"""Cost of the perceptual (VGG16 feature) term at the CIFAR shape: batch 256, 32 x 32, real VGG16 widths (default-init weights: the
arithmetic does not depend on the values), fp32.

Times the conv Sphere Encoder step (hidden 32..512, L = 128, UPGrad) without and with the term, eager (train.train_step) and replayed
(train.GraphedTrainStep), and counts the kernel nodes of each captured graph; times the term alone -- PerceptualLoss forward + backward to
the prediction -- against the torch composition (F.conv2d / F.max_pool2d / F.mse_loss, NCHW) on the same device and weights (median of
--repeats windows, alternating the two); and times the normalisation and the two pools alone, reported as bandwidth against their
algorithmic byte counts.  Prints one JSON line.  bench.py's fixed configurations are not touched.

Usage:  python tools/perceptual_bench.py [--steps 20] [--warmup 3] [--repeats 5]
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--latent", type=int, default=128)
    ap.add_argument("--agg", default="upgrad")
    a = ap.parse_args()

    import torch
    import torch.nn.functional as F

    import movae_amd  # noqa: F401
    from movae_amd import aggregation, ops, perceptual
    from movae_amd.models import build_sphere_encoder
    from movae_amd.train import GraphedTrainStep, make_optimizer, train_step

    dev = torch.device("cuda:0")
    B, L = a.batch, a.latent
    args = Args(batch_size=B, dataset_size=50000, recons_objective="mse", recons_activation=None, latent_dim=L,
                hidden_dims=[32, 64, 128, 256, 512], aggregator=a.agg, agg_norm_eps=1e-4, agg_reg_eps=1e-4, mgda_epsilon=1e-5,
                mgda_max_iters=250, pref_weights=None, optimizer="adam", lr=1e-3, wd=0, momentum=0.9, max_grad_norm=None)
    x = torch.rand(B, 3, 32, 32, generator=torch.Generator().manual_seed(0)).to(dev)
    res = {"arch": "sphere_encoder", "batch": B, "agg": a.agg, "shape": f"CIFAR (32x32, hidden 32..512, L {L}, VGG16 widths, fp32)"}
    torch.manual_seed(0)
    vgg = perceptual.PerceptualLoss().state_dict()

    def fresh(term):
        torch.manual_seed(0)
        perceptual.use_vgg16_weights(vgg if term else None)
        net = build_sphere_encoder(32, 3, args, dev, use_perceptual=term).to(dev).train()
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

    # ---- the step without and with the term: eager, then captured ------------------------------------------------------------------
    for term, tag in ((False, "plain"), (True, "perceptual")):
        net, opt, agg = fresh(term)
        for _ in range(a.warmup):
            train_step(net, x, opt, agg, args)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            train_step(net, x, opt, agg, args)
        torch.cuda.synchronize()
        res[f"{tag}_eager_ms_per_step"] = (time.perf_counter() - t0) / a.steps * 1e3
        net, opt, agg = fresh(term)
        orig, torch.cuda.CUDAGraph = torch.cuda.CUDAGraph, KeptGraph
        try:
            gs = GraphedTrainStep(net, opt, agg, args, x, warmup=3)
        finally:
            torch.cuda.CUDAGraph = orig
        res[f"{tag}_graphed_kernels_per_step"] = kernel_nodes(gs.graph)
        for _ in range(a.warmup):
            gs.step(x)
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.steps):
            gs.step(x)
        end.record()
        torch.cuda.synchronize()
        res[f"{tag}_graphed_ms_per_step"] = start.elapsed_time(end) / a.steps
        res[f"{tag}_finite"] = all(math.isfinite(float(v.item())) for v in gs.loss_dict.values())
        del gs, net, opt
    perceptual.use_vgg16_weights(None)

    def window(fn, iters):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / iters * 1e3  # us per call, eager launches

    def versus(name, hip_fn, torch_fn, iters):
        for fn in (hip_fn, torch_fn):
            window(fn, 3)
        th, tt = [], []
        for _ in range(a.repeats):  # alternate the two
            th.append(window(hip_fn, iters))
            tt.append(window(torch_fn, iters))
        res[f"{name}_hip_us"], res[f"{name}_torch_us"] = statistics.median(th), statistics.median(tt)
        res[f"{name}_hip_us_spread"], res[f"{name}_torch_us_spread"] = [min(th), max(th)], [min(tt), max(tt)]
        return res[f"{name}_hip_us"]

    # ---- the term alone against the torch composition ---------------------------------------------------------------------------------
    pl = perceptual.PerceptualLoss(vgg, device=dev)
    g = torch.Generator().manual_seed(1)
    pred = torch.tanh(torch.randn(B, 32, 32, 3, generator=g)).to(dev).requires_grad_(True)  # an NHWC buffer, as the decoder writes it
    target = torch.rand(B, 32, 32, 3, generator=g).to(dev)
    pred_v, target_v = pred.permute(0, 3, 1, 2), target.permute(0, 3, 1, 2)  # their logical NCHW views
    pred_t, target_t = pred.detach().permute(0, 3, 1, 2).contiguous().requires_grad_(True), target.permute(0, 3, 1, 2).contiguous()
    wt = [(vgg[f"features.{n}.weight"].to(dev), vgg[f"features.{n}.bias"].to(dev)) for n in perceptual.CONV_INDICES]
    mean, std = torch.tensor([0.485, 0.456, 0.406], device=dev).view(1, 3, 1, 1), torch.tensor([0.229, 0.224, 0.225], device=dev).view(1, 3, 1, 1)

    def norm_t(t):  # utils/objectives.py:66-72 (with its host sync)
        if t.min() < 0:
            t = (t + 1) / 2
        return (torch.clamp(t, 0, 1) - mean) / std

    def feats_t(t):
        for n, (w, b) in zip(perceptual.CONV_INDICES, wt):
            t = F.relu(F.conv2d(t, w, b, padding=1))
            if n in perceptual.POOL_AFTER:
                t = F.max_pool2d(t, 2, 2)
        return t

    def term_torch():
        with torch.no_grad():
            ft = feats_t(norm_t(target_t))
        return torch.autograd.grad(F.mse_loss(feats_t(norm_t(pred_t)), ft), pred_t)[0]

    def term_hip():
        return torch.autograd.grad(pl(pred_v, target_v), pred)[0]

    versus("term", term_hip, term_torch, 10)

    # ---- the normalisation and the pools alone, against their byte counts -------------------------------------------------------------
    imgs = [torch.tanh(torch.randn(B, 32, 32, 3, generator=g)).to(dev).requires_grad_(True) for _ in range(3)]
    cots = [torch.randn(B, 32, 32, 3, generator=g).to(dev) for _ in range(3)]
    n = imgs[0].numel()

    def prep_hip():
        return torch.autograd.grad(ops.vgg_prep(*imgs), imgs, cots)

    def prep_torch():
        return torch.autograd.grad([norm_t(t.permute(0, 3, 1, 2)) for t in imgs], imgs, [c.permute(0, 3, 1, 2) for c in cots])

    us = versus("prep3", prep_hip, prep_torch, 50)
    res["prep3_bytes"] = 3 * 24 * n  # per tensor 12 n forward (flag pass 4 n, normalise 8 n) + 12 n backward
    res["prep3_hip_GBps"] = res["prep3_bytes"] / (us * 1e-6) / 1e9
    for c, hw in ((64, 32), (128, 16)):
        xp = torch.relu(torch.randn(B, hw, hw, c, generator=g)).to(dev).requires_grad_(True)
        xp_t = xp.detach().permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        dy = torch.randn(B, hw // 2, hw // 2, c, generator=g).to(dev)
        dy_t = dy.permute(0, 3, 1, 2)
        us = versus(f"pool{c}", lambda: torch.autograd.grad(ops.max_pool2x2(xp), xp, dy),
                    lambda: torch.autograd.grad(F.max_pool2d(xp_t, 2, 2), xp_t, dy_t), 50)
        p = dy.numel()
        res[f"pool{c}_bytes"] = 4 * (4 * p + p) + 4 * (p + p + 4 * p + 4 * p)  # forward 16 P + 4 P; backward 4 P + 4 P + 16 P read, 16 P written
        res[f"pool{c}_hip_GBps"] = res[f"pool{c}_bytes"] / (us * 1e-6) / 1e9
    print(json.dumps(res))


if __name__ == "__main__":
    main()

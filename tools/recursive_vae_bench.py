#!/usr/bin/env python3
"""Step time of the recursive-cyclic VAE (rc_vae) at the C2 shape: batch 256, 32 x 32, hidden 32..512, latent 128, UPGrad, fp32.

Times the eager step (train.train_step) and the captured step (train.GraphedTrainStep replay), each with the batched Jacobian
(autojac.BATCHED_VJP: the K rows pulled back in one traversal) and the sequential one (one autograd pass per loss), and counts the
kernel nodes of the captured graph -- the launches one replayed step makes (the same unit for --arch vae, the C2 step).  Prints
one JSON line.  bench.py's fixed configurations are not touched.

Usage:  python tools/recursive_vae_bench.py [--arch rc_vae] [--steps 30] [--warmup 5]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Args:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="rc_vae", choices=["rc_vae", "recursive_kl_vae", "cycle_vae", "vae"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--agg", default="upgrad")
    a = ap.parse_args()

    import torch

    import movae_amd  # noqa: F401
    from movae_amd import aggregation, autojac
    from movae_amd.models import get_network
    from movae_amd.train import GraphedTrainStep, make_optimizer, train_step

    dev = torch.device("cuda:0")
    lw = {"rc_vae": [1.0, 0.00025, 0.00025], "recursive_kl_vae": [1.0, 0.00025], "cycle_vae": [1.0, 0.00025], "vae": None}[a.arch]
    B = a.batch
    args = Args(arch=a.arch, batch_size=B, dataset_size=50000, recons_objective="mse", recons_activation=None, loss_weights=lw,
                latent_dim=128, hidden_dims=[32, 64, 128, 256, 512], recursive_kld_anneal_steps=25000, aggregator=a.agg,
                agg_norm_eps=1e-4, agg_reg_eps=1e-4, mgda_epsilon=1e-5, mgda_max_iters=250, pref_weights=None, optimizer="adam",
                lr=1e-3, wd=0, momentum=0.9, max_grad_norm=None)
    x = torch.rand(B, 3, 32, 32, generator=torch.Generator().manual_seed(0)).to(dev)
    res = {"arch": a.arch, "batch": B, "agg": a.agg, "shape": "C2 (32x32, hidden 32..512, latent 128, fp32)"}

    def fresh():
        torch.manual_seed(0)
        net = get_network(32, 3, args, dev).to(dev).train()
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

    for batched in (True, False):
        tag = "batched" if batched else "sequential"
        autojac.BATCHED_VJP = batched  # (the multi-pass VAEs read MOVAE_BATCHED_FULL_JACOBIAN: set from the same switch here)
        autojac.BATCHED_FULL_JACOBIAN = batched
        # ---- eager ------------------------------------------------------------------------------------------------------
        net, opt, agg = fresh()
        for _ in range(a.warmup):
            train_step(net, x, opt, agg, args)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            train_step(net, x, opt, agg, args)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / a.steps * 1e3
        res[f"eager_{tag}_ms_per_step"], res[f"eager_{tag}_images_per_s"] = ms, B / (ms * 1e-3)
        # ---- graphed ----------------------------------------------------------------------------------------------------
        net, opt, agg = fresh()
        orig, torch.cuda.CUDAGraph = torch.cuda.CUDAGraph, KeptGraph
        try:
            gs = GraphedTrainStep(net, opt, agg, args, x, warmup=3)
        finally:
            torch.cuda.CUDAGraph = orig
        res[f"graphed_{tag}_kernels_per_step"] = kernel_nodes(gs.graph)
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
        res[f"graphed_{tag}_ms_per_step"], res[f"graphed_{tag}_images_per_s"] = ms, B / (ms * 1e-3)
        loss = {k: float(v.item()) for k, v in gs.loss_dict.items()}
        res[f"{tag}_finite"] = all(v == v and abs(v) < float("inf") for v in loss.values())
        del gs, net, opt
    print(json.dumps(res))


if __name__ == "__main__":
    main()

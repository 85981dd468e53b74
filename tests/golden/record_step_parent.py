#!/usr/bin/env python3
"""Recorder of tests/golden/step_parent.json: what one optimisation step of the tiny VAE, VQ-VAE, VQ-VAE-2 and BetaTC-VAE
configurations (the networks of tests/golden/<tag>.npz at batch 4, UPGrad, Adam) LAUNCHES and COMPUTES on an MI355X, per configuration:

  calls        the names, in order, of the C-ABI calls of one captured step (train.GraphedTrainStep(record_calls=True).calls)
  defer_stats  movae_reduce_defer_stats' (parked, carried, launched alone) after one eager step, and what is still pending
  params       SHA-256 of every parameter after three replays of the captured step from the fixture's seed (preserve_state: the
               first replay is step 1; the reparameterisation noise comes from the kernel's own generator, seeded by that seed)

The committed file was recorded at commit 58d610d ("Use a saved run ..."), the last one before the step's host-side state (the
Jacobian arena, the persistent zero gradients, the output-activation link, VQ-VAE-2's lazily formed sums) moved from process-wide
registries to the objects that use it; test_step_parent.py replays the same on the current tree and holds it to every recorded
field.  Only host code changed between the two, the kernels fold in a fixed order and use no float atomics, so the parameters
are recorded as digests of their bytes.

Usage:  python tests/golden/record_step_parent.py tests/golden/step_parent.json
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TAGS = ["vae_tiny", "vq_vae_tiny", "vq_vae2_tiny", "betatc_vae_tiny"]
BATCH, REPLAYS = 4, 3


class Args:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def make(tag, dev):
    """(net, args, x): the fixture's network drawn from the fixture's seed, on the device, in training mode; a batch of BATCH images."""
    import ast

    from movae_amd.models import get_network
    from movae_amd.models.betatc_vae import BetaTCVAE

    fx = np.load(os.path.join(HERE, tag + ".npz"))
    m = dict(str(s).split("=", 1) for s in fx["meta"])
    kw = {k: int(m[k]) for k in ("latent_dim", "embedding_dim", "num_embeddings", "num_residual_layers", "anneal_steps") if k in m}
    if "hidden_dims" in m:
        kw["hidden_dims"] = list(ast.literal_eval(m["hidden_dims"]))
    a = Args(arch=m["arch"], batch_size=BATCH, dataset_size=int(m["dataset_size"]), recons_objective=m.get("objective", "mse"),
             recons_activation=None, loss_weights=None, aggregator="upgrad", agg_norm_eps=1e-4, agg_reg_eps=1e-4, mgda_epsilon=1e-5,
             mgda_max_iters=250, pref_weights=None, optimizer="adam", lr=1e-3, wd=0, momentum=0.9, max_grad_norm=None, **kw)
    torch.manual_seed(int(m["seed"]))
    BetaTCVAE.num_iter = 0
    net = get_network(int(m["input_size"]), num_channels=3, args=a, device=dev).to(dev).train()
    size = int(m["input_size"])
    return net, a, torch.rand(BATCH, 3, size, size, generator=torch.Generator().manual_seed(int(m["seed"]) + 1)).to(dev)


def graphed_step(tag, dev, record_calls=False):
    """A GraphedTrainStep on a freshly drawn copy of the fixture's network, its warm-up rewound -> (step, x)."""
    from movae_amd import aggregation
    from movae_amd.train import GraphedTrainStep, make_optimizer

    net, a, x = make(tag, dev)
    opt = make_optimizer(net, a, capturable=True)
    return GraphedTrainStep(net, opt, aggregation.make_aggregator(a), a, x, warmup=3, record_calls=record_calls, preserve_state=True), x


def replayed_params(gs, x):
    for _ in range(REPLAYS):
        gs.step(x)
    torch.cuda.synchronize()
    return {n: sha(p) for n, p in gs.net.named_parameters()}


def record(tag, dev):
    from movae_amd import _lib as L
    from movae_amd import aggregation
    from movae_amd.models.betatc_vae import BetaTCVAE
    from movae_amd.train import make_optimizer, train_step

    lib = L.load()
    net, a, x = make(tag, dev)
    stats = (C.c_longlong * 3)()
    lib.movae_reduce_defer_stats(stats, 1)
    train_step(net, x, make_optimizer(net, a), aggregation.make_aggregator(a), a)
    torch.cuda.synchronize()
    pending = lib.movae_reduce_defer_stats(stats, 0)
    gs, x = graphed_step(tag, dev, record_calls=True)
    rec = {"calls": [name for name, _ in gs.calls], "defer_stats": list(stats) + [pending], "params": replayed_params(gs, x)}
    BetaTCVAE.num_iter = 0
    return rec


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import movae_amd  # noqa: F401

    dev = torch.device("cuda:0")
    rec = {tag: record(tag, dev) for tag in TAGS}
    with open(sys.argv[1], "w") as fh:
        json.dump({"cases": rec}, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print("recorded", sys.argv[1], {t: len(r["calls"]) for t, r in rec.items()}, os.path.getsize(sys.argv[1]), "bytes")


if __name__ == "__main__":
    main()

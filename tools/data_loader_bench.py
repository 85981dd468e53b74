#!/usr/bin/env python3
"""What the device batch loader (movae_amd/data.py, csrc/data.hip) costs and saves at the C2 shape (CIFAR-10 VAE, --agg upgrad, batch 256):

  * one epoch of train.train_epoch -- main.py's loop -- over a ResidentImages set of CIFAR-10's size (50 000 x 32 x 32 x 3 uint8),
    with the device loader and with the host DataLoader (--data_loader host) over the SAME set, each with the eager and with the
    graphed step: host clock around whole epochs that end in a device synchronise, after a warm-up epoch (which also captures the
    graph); medians of --repeats windows, the four variants alternating.  A window of a device-loader variant is --device_epochs
    epochs and a window of a host-loader variant --host_steps steps (default: one epoch of 196), so that each lasts a second or more;
  * movae_batch_u8 alone at that shape: device events around --iters eager launches, as us per call and achieved bytes/s against
    the b h w c bytes read + 4 b h w c bytes written;
  * the C-ABI calls of one captured step on the loader's batch (a logical-NCHW view of an NHWC buffer) and on its contiguous NCHW
    copy -- the form every batch had before the device loader -- from GraphedTrainStep(record_calls=True).

The pixels are seeded noise unless --data_dir holds cifar-10-batches-py: the cost of a batch does not depend on the values.
Prints one JSON line.  bench.py is not touched.

Usage:  python tools/data_loader_bench.py [--repeats 3] [--device_epochs 5] [--host_steps 196]
"""
import argparse
import collections
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device_epochs", type=int, default=5)
    ap.add_argument("--host_steps", type=int, default=196)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--data_dir", type=str, default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    import movae_amd  # noqa: F401
    from movae_amd import _lib as L
    from movae_amd import aggregation, data, ops, train
    from movae_amd.models import get_network

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    if a.data_dir:
        ds = train.get_dataset("cifar10", data_dir=a.data_dir)[0]
    else:
        ds = data.ResidentImages(np.random.default_rng(0).integers(0, 256, size=(a.n, 32, 32, 3), dtype=np.uint8), False, train=True)
    batch = 256
    steps = -(-len(ds) // batch)
    res = {"config": "C2: --arch vae --agg upgrad --batch_size 256, 32x32", "images": len(ds), "steps_per_epoch": steps}

    def variant(loader_mode, graph):
        argv = ["--dataset", "CIFAR10", "--arch", "vae", "--agg", "upgrad", "--batch_size", str(batch), "--seed", "0", "--device", "cuda:0",
                "--graph", graph, "--data_loader", loader_mode]
        args = train.parse_args(argv)
        args.dataset_size = len(ds)
        torch.manual_seed(0)
        net = get_network(32, num_channels=3, args=args, device=dev).to(dev)
        agg = aggregation.make_aggregator(args)
        graphed = {"batch": batch, "step": None} if graph == "on" else None
        opt = train.make_optimizer(net, args, capturable=graphed is not None)
        loader = train.make_loader(ds, batch, dev, args, shuffle=True)
        state = {"epoch": 0, "step": 0}

        def run(epochs, max_steps=None):
            """-> (seconds, steps made)"""
            torch.cuda.synchronize()
            t0, s0 = time.perf_counter(), state["step"]
            for _ in range(epochs):
                state["epoch"] += 1
                if isinstance(loader, data.DeviceBatchLoader):
                    loader.set_epoch(state["epoch"])
                else:
                    ds.set_epoch(state["epoch"])
                args.max_steps = None if max_steps is None else state["step"] + max_steps
                _, state["step"] = train.train_epoch(net, loader, opt, agg, state["step"], dev, args, None, None, graphed)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, state["step"] - s0

        return run

    names = [("device", "off"), ("device", "on"), ("host", "off"), ("host", "on")]
    runs = {k: variant(*k) for k in names}
    for k, run in runs.items():  # warm-up: code objects, the capture, the upload of the set
        run(1, None if k[0] == "device" else a.host_steps)
    times = collections.defaultdict(list)
    for _ in range(a.repeats):
        for k, run in runs.items():
            dt, made = run(a.device_epochs, None) if k[0] == "device" else run(1, a.host_steps)
            times[k].append(dt / made * 1e3)  # ms per step, loader included
    for k in names:
        ms = statistics.median(times[k])
        tag = f"{k[0]}_loader_{'graphed' if k[1] == 'on' else 'eager'}"
        res[tag] = {"ms_per_step": ms, "spread_ms": [min(times[k]), max(times[k])], "epoch_s": ms * steps / 1e3,
                    "img_per_s": batch / (ms / 1e3), "steps_per_window": a.device_epochs * steps if k[0] == "device" else a.host_steps}

    # ---- the kernel alone ----
    loader = data.DeviceBatchLoader(ds, batch, dev, shuffle=True)
    x, _ = next(iter(loader))
    rows = loader._device_indices()[:batch]

    def window(iters):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            ops.batch_u8(loader._store, rows, loader._lut, True, 0, 0)
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / iters * 1e3

    window(50)
    us = [window(a.iters) for _ in range(a.repeats)]
    moved = 5 * batch * 32 * 32 * 3
    res["movae_batch_u8_eager"] = {"us_per_call": statistics.median(us), "spread_us": [min(us), max(us)], "bytes": moved,
                                   "GBps": moved / (statistics.median(us) * 1e-6) / 1e9,
                                   "note": "back-to-back eager launches, allocation of the output included: launch-bound"}

    # ---- calls of one captured step: the loader's view against the contiguous NCHW batch ----
    def calls_of(example):
        args = train.parse_args(["--arch", "vae", "--agg", "upgrad", "--batch_size", str(batch), "--device", "cuda:0"])
        args.dataset_size = len(ds)
        torch.manual_seed(0)
        net = get_network(32, num_channels=3, args=args, device=dev).to(dev)
        opt = train.make_optimizer(net, args, capturable=True)
        gs = train.GraphedTrainStep(net, opt, aggregation.make_aggregator(args), args, example, record_calls=True)
        return collections.Counter(name for name, _ in gs.calls)

    view, copy = calls_of(x), calls_of(x.contiguous())
    res["calls_per_captured_step"] = {"loader_view": sum(view.values()), "contiguous_nchw": sum(copy.values()),
                                      "only_in_contiguous": dict(copy - view), "only_in_view": dict(view - copy)}
    L.defer_flush()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

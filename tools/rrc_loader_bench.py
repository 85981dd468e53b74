#!/usr/bin/env python3
"""What the RandomResizedCrop device loader (movae_amd/data.py: RaggedBatchLoader, csrc/data.hip: movae_batch_rrc_u8) costs, on a synthetic
ragged set of oxford-flower-102's shape: --n (2 040) images of h = 500 and w uniform in 500 .. 750, about 2 GB as uint8, output side 256.

  * movae_batch_rrc_u8 alone at B = --kernel_batch (64) and at the training batch: one device-event pair around every one of --iters
    eager launches over the epoch's own batches, the median in us per call, and the achieved bytes/s against (crop bytes read +
    4 B s^2 3 bytes written);
  * images/s of one epoch of train.train_epoch -- main.py's loop -- for a VQ-VAE-2 at the C4 shape (--batch_size 8, --agg mgda_ln) with
    the device loader, and with the host DataLoader (--data_loader host --num_workers W) over the SAME set: host clock around whole
    epochs that end in a device synchronise, after a warm-up epoch; medians of --repeats epochs, the variants alternating, in one
    process like tools/data_loader_bench.py.  Host epochs may be cut to --host_steps steps.  The host path is bound by its workers'
    resample, so give it the cores it can really have: W workers plus the main process and the pinning thread should fit the CPUs
    of the run, and the line records W.

The pixels are a tiled block of seeded noise: the cost of a batch does not depend on the values.  Prints one JSON line.

Usage:  python tools/rrc_loader_bench.py [--repeats 3] [--num_workers 16] [--host_steps 0]
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
    ap.add_argument("--n", type=int, default=2040)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--kernel_batch", type=int, default=64)
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--num_workers", type=int, default=16)
    ap.add_argument("--host_steps", type=int, default=0, help="steps per timed host-loader window (0: the whole epoch)")
    ap.add_argument("--graph", choices=["on", "off"], default="on")
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
    size = 256
    rng = np.random.default_rng(0)
    w = rng.integers(500, 751, size=a.n)
    index = np.zeros((a.n, 3), dtype=np.int64)
    index[:, 1], index[:, 2] = 500, w
    index[1:, 0] = np.cumsum(3 * index[:-1, 1] * index[:-1, 2])
    total = int(index[-1, 0] + 3 * index[-1, 1] * index[-1, 2])
    block = rng.integers(0, 256, size=1 << 24, dtype=np.uint8)
    blob = np.tile(block, -(-total // block.size))[:total]
    ds = data.RaggedImages(blob, index, size, False, train=True, seed=0)
    res = {"images": a.n, "blob_bytes": total, "side": size, "kmax": ds.kmax,
           "config": f"C4 shape: --arch vq_vae2 --agg mgda_ln --batch_size {a.batch_size}, 256x256, --graph {a.graph}"}

    # ---- the kernel alone, at the measurement batch and at the training batch ----
    def kernel_alone(batch):
        loader = data.RaggedBatchLoader(ds, batch, dev, shuffle=True)
        rows_all, host_rows, boxes = loader._device_indices(), loader.indices(), ds.boxes(0)
        starts = range(0, a.n - batch + 1, batch)
        batches = [rows_all[s:s + batch] for s in starts]
        crop_bytes = [int((3 * boxes[host_rows[s:s + batch], 2].astype(np.int64) * boxes[host_rows[s:s + batch], 3]).sum()) for s in starts]

        def one(k):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            ops.batch_rrc_u8(loader._store, loader._offsets, loader._dims, loader._boxes, batches[k % len(batches)], size, 3, ds.kmax,
                             loader._lut, True, 0, 0)
            end.record()
            return start, end

        for k in range(20):
            one(k)
        torch.cuda.synchronize()
        pairs = [one(k) for k in range(a.iters)]
        torch.cuda.synchronize()
        us = [s.elapsed_time(e) * 1e3 for s, e in pairs]
        med, written = statistics.median(us), 4 * batch * size * size * 3
        return loader, {"batch": batch, "us_per_call": med, "spread_us": [min(us), max(us)], "crop_bytes_read": statistics.mean(crop_bytes),
                        "bytes_written": written, "GBps": (statistics.mean(crop_bytes) + written) / (med * 1e-6) / 1e9,
                        "us_per_image": med / batch, "note": "one event pair per eager launch, allocation of the output included"}

    keep, res["movae_batch_rrc_u8"] = kernel_alone(a.kernel_batch)  # (kept: the loaders below share its copy of the blob)
    _, res["movae_batch_rrc_u8_train_batch"] = kernel_alone(a.batch_size)

    # ---- an epoch of the training loop, device loader against host loader ----
    steps = -(-a.n // a.batch_size)

    def variant(loader_mode):
        argv = ["--dataset", "oxford-flower-102", "--arch", "vq_vae2", "--agg", "mgda_ln", "--batch_size", str(a.batch_size), "--seed", "0",
                "--device", "cuda:0", "--embedding_dim", "64", "--num_embeddings", "512", "--hidden_dims", "128", "256",
                "--num_residual_layers", "2", "--graph", a.graph, "--data_loader", loader_mode, "--num_workers", str(a.num_workers)]
        args = train.parse_args(argv)
        args.dataset_size = len(ds)
        torch.manual_seed(0)
        net = get_network(size, num_channels=3, args=args, device=dev).to(dev)
        agg = aggregation.make_aggregator(args)
        graphed = {"batch": a.batch_size, "step": None} if a.graph == "on" and getattr(net, "graph_safe", False) else None
        opt = train.make_optimizer(net, args, capturable=graphed is not None)
        ld = train.make_loader(ds, a.batch_size, dev, args, shuffle=True)
        state = {"epoch": 0, "step": 0}

        def run(max_steps=None):
            """One epoch (or its first max_steps steps) -> (seconds, steps made)."""
            torch.cuda.synchronize()
            t0, s0 = time.perf_counter(), state["step"]
            state["epoch"] += 1
            if isinstance(ld, data.ResidentLoader):
                ld.set_epoch(state["epoch"])
            else:
                ds.set_epoch(state["epoch"])
            args.max_steps = None if not max_steps else state["step"] + max_steps
            _, state["step"] = train.train_epoch(net, ld, opt, agg, state["step"], dev, args, None, None, graphed)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, state["step"] - s0

        return run, graphed is not None

    names = ["device", "host"]
    runs = {k: variant(k) for k in names}
    for k in names:  # warm-up: code objects, the capture, the upload of the set, the first workers
        runs[k][0](None if k == "device" else (a.host_steps or 32))
    times = collections.defaultdict(list)
    for _ in range(a.repeats):
        for k in names:
            dt, made = runs[k][0](None if k == "device" else a.host_steps)
            times[k].append(dt / made * 1e3)  # ms per step, loader included
    for k in names:
        ms = statistics.median(times[k])
        res[f"{k}_loader"] = {"ms_per_step": ms, "spread_ms": [min(times[k]), max(times[k])], "epoch_s": ms * steps / 1e3,
                              "img_per_s": a.batch_size / (ms / 1e3), "graphed": runs[k][1],
                              **({"num_workers": a.num_workers} if k == "host" else {})}
    L.defer_flush()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

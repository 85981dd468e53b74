#!/usr/bin/env python3
"""What the streamed loader (movae_amd/data.py: StreamedBatchLoader, csrc/data.hip: movae_batch_u8_staged) costs at the ImageNet shape,
in one process, on a seeded synthetic set that FITS the device so that the resident loader can be its yardstick: --n (8 192) images of
256 x 256 x 3 in 4 shards, written as .npy files into a scratch folder and opened as maps like the reader opens them.  The files
have just been written, so THE PAGE CACHE IS WARM: this is the rate from host memory; cold-cache and on-disk rates are not measured.

  (a) the loaders alone at batch 128: whole epochs under a host clock, ended by a device synchronise, after a warm-up epoch --
      streamed with 1 / 4 / 8 gather threads, data.DeviceBatchLoader over the concatenated array, and the host DataLoader
      (--data_loader host) with 1 / 4 / 8 worker processes (its window cut to --host_batches batches; each batch is moved to the
      device like train_epoch moves it).  Images/s, median and range of --repeats windows, the variants alternating.  Separately, by
      device events per batch over the loader's own slots and staging buffer: the host-to-device copy and the convert launch.
  (b) one training epoch (train.train_epoch) of the configs/imagenet/vq_vae model (hidden 128 / 256, K 512, D 64, UPGrad, Adam,
      batch 128, fp32, --graph auto): resident against streamed (--workers gather threads), alternating, --repeats windows each after
      a warm-up epoch (which captures the graph); the streamed rate as a fraction of the resident one.

Prints one JSON line.  bench.py is not touched.

Usage:  python tools/stream_loader_bench.py [--repeats 3] [--n 8192] [--workers 4] [--skip_training]
"""
import argparse
import collections
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--shards", type=int, default=4)
    ap.add_argument("--batch_size", type=int, default=128)
    ap.add_argument("--workers", type=int, default=4, help="gather threads of the streamed training epochs")
    ap.add_argument("--host_batches", type=int, default=8, help="batches per window of the host DataLoader")
    ap.add_argument("--event_batches", type=int, default=32)
    ap.add_argument("--dir", type=str, default=None, help="where the shards are written (default: a temporary folder, removed at the end)")
    ap.add_argument("--skip_training", action="store_true")
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
    size, batch = 256, a.batch_size
    folder = a.dir or tempfile.mkdtemp(prefix="movae_stream_bench_")
    os.makedirs(folder, exist_ok=True)
    try:
        # seeded noise; the cost of a batch does not depend on the values, so one block of 256 images is rolled to fill the set
        block = np.random.default_rng(0).integers(0, 256, size=(256, size, size, 3), dtype=np.uint8)
        whole = np.empty((a.n, size, size, 3), dtype=np.uint8)
        for s in range(0, a.n, 256):
            whole[s:s + 256] = np.roll(block, s // 256, axis=2)[:a.n - s]
        per = -(-a.n // a.shards)
        paths = []
        for k in range(a.shards):
            paths.append(os.path.join(folder, f"imagenet_train_u8_{k:05d}.npy"))
            np.save(paths[-1], whole[k * per:(k + 1) * per])
        maps = [np.load(p, mmap_mode="r") for p in paths]
        sharded = data.ShardedImages(maps, True, train=True, seed=0)
        resident = data.ResidentImages(whole, True, train=True, seed=0)
        steps = -(-a.n // batch)
        res = {"shape": f"{a.n} x {size} x {size} x 3 uint8 in {a.shards} shards, batch {batch}, page cache warm", "batches_per_epoch": steps}

        # ---- (a) the loaders alone ----
        def epoch_of(loader, ds, limit=None):
            state = {"epoch": 0}

            def run():
                state["epoch"] += 1
                if isinstance(loader, data.ResidentLoader):
                    loader.set_epoch(state["epoch"])
                else:
                    ds.set_epoch(state["epoch"])
                torch.cuda.synchronize()
                t0, images = time.perf_counter(), 0
                for k, (x, _) in enumerate(loader):
                    x = x.to(dev, non_blocking=True)
                    images += x.size(0)
                    if limit is not None and k + 1 >= limit:
                        break
                torch.cuda.synchronize()
                return images / (time.perf_counter() - t0)

            return run

        host_args = lambda w: train.parse_args(["--data_loader", "host", "--num_workers", str(w)])  # noqa: E731
        runs = collections.OrderedDict()
        for w in (1, 4, 8):
            runs[f"streamed_{w}_threads"] = epoch_of(data.StreamedBatchLoader(sharded, batch, dev, True, num_workers=w), sharded)
        runs["device_resident"] = epoch_of(data.DeviceBatchLoader(resident, batch, dev, True), resident)
        for w in (1, 4, 8):
            runs[f"host_dataloader_{w}_workers"] = epoch_of(train.make_loader(sharded, batch, dev, host_args(w), shuffle=True), sharded,
                                                            limit=a.host_batches)
        rates = collections.defaultdict(list)
        for name, run in runs.items():  # warm-up: code objects, the upload of the resident set, the pinned ring
            run()
        for _ in range(a.repeats):
            for name, run in runs.items():
                rates[name].append(run())
        res["loaders_alone_img_per_s"] = {k: {"median": statistics.median(v), "range": [min(v), max(v)]} for k, v in rates.items()}
        res["loaders_alone_note"] = (f"whole epochs of {steps} batches; the host DataLoader's windows are its first {a.host_batches} batches, "
                                     f"worker start-up included")

        # ---- the device step of a streamed batch, by events: the copy and the launch ----
        loader = data.StreamedBatchLoader(sharded, batch, dev, True, num_workers=4)
        next(iter(loader))  # allocates the ring and the staging buffer, fills slot 0
        ids = loader._device_indices()[:batch]
        copy_us, convert_us = [], []
        for k in range(a.event_batches + 4):
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            loader._stage.copy_(loader._slots[k % loader.depth], non_blocking=True)
            e1.record()
            ops.batch_u8_staged(loader._stage, ids, loader._lut, True, 0, 1)
            e2.record()
            torch.cuda.synchronize()
            if k >= 4:
                copy_us.append(e0.elapsed_time(e1) * 1e3)
                convert_us.append(e1.elapsed_time(e2) * 1e3)
        nbytes = batch * size * size * 3
        res["device_step_per_batch"] = {
            "copy_us": {"median": statistics.median(copy_us), "range": [min(copy_us), max(copy_us)], "bytes": nbytes,
                        "GBps": nbytes / (statistics.median(copy_us) * 1e-6) / 1e9},
            "convert_us": {"median": statistics.median(convert_us), "range": [min(convert_us), max(convert_us)], "bytes": 5 * nbytes,
                           "GBps": 5 * nbytes / (statistics.median(convert_us) * 1e-6) / 1e9}}
        # and the gather alone, one thread, into a pinned slot
        order = np.asarray(loader.indices())
        gather_ms = []
        for k in range(min(16, steps - 1)):  # another batch of the epoch every time: rows that are not in the caches from the last call
            rows = order[k * batch:(k + 1) * batch]
            t0 = time.perf_counter()
            sharded.gather(rows, loader._slots_np[k % loader.depth][:rows.shape[0]])
            gather_ms.append((time.perf_counter() - t0) * 1e3)
        res["gather_ms_per_batch_one_thread"] = {"median": statistics.median(gather_ms), "range": [min(gather_ms), max(gather_ms)]}
        del loader

        # ---- (b) a training epoch ----
        if not a.skip_training:
            def variant(ds, mode):
                argv = ["--dataset", "imagenet", "--arch", "vq_vae", "--hidden_dims", "128", "256", "--embedding_dim", "64",
                        "--num_embeddings", "512", "--agg", "upgrad", "--optimizer", "adam", "--lr", "1e-4", "--batch_size", str(batch),
                        "--normalize_inputs", "--seed", "42", "--device", "cuda:0", "--graph", "auto", "--data_loader", mode,
                        "--num_workers", str(a.workers)]
                args = train.parse_args(argv)
                args.dataset_size = len(ds)
                torch.manual_seed(0)
                net = get_network(size, num_channels=3, args=args, device=dev).to(dev)
                agg = aggregation.make_aggregator(args)
                graphed = {"batch": batch, "step": None}
                opt = train.make_optimizer(net, args, capturable=True)
                ld = train.make_loader(ds, batch, dev, args, shuffle=True)
                state = {"epoch": 0, "step": 0}

                def run():
                    state["epoch"] += 1
                    ld.set_epoch(state["epoch"])
                    torch.cuda.synchronize()
                    t0, s0 = time.perf_counter(), state["step"]
                    _, state["step"] = train.train_epoch(net, ld, opt, agg, state["step"], dev, args, None, None, graphed)
                    torch.cuda.synchronize()
                    return (state["step"] - s0) * batch / (time.perf_counter() - t0), graphed

                return run

            tr = collections.OrderedDict(resident=variant(resident, "device"), streamed=variant(sharded, "stream"))
            forms = {}
            for name, run in tr.items():
                _, g = run()  # warm-up: the capture
                forms[name] = "graphed" if g.get("step") is not None else "eager"
            rates = collections.defaultdict(list)
            for _ in range(a.repeats):
                for name, run in tr.items():
                    rates[name].append(run()[0])
            med = {k: statistics.median(v) for k, v in rates.items()}
            res["training_epoch_img_per_s"] = {k: {"median": med[k], "range": [min(v), max(v)], "all": v, "step": forms[k],
                                                   "ms_per_step": batch / med[k] * 1e3} for k, v in rates.items()}
            res["training_streamed_over_resident"] = med["streamed"] / med["resident"]
            res["training_note"] = f"vq_vae 128/256, K 512, D 64, upgrad, adam, fp32, --graph auto; {a.workers} gather threads; {steps} steps per epoch"
        L.defer_flush()
        print(json.dumps(res))
    finally:
        if a.dir is None:
            shutil.rmtree(folder, ignore_errors=True)


if __name__ == "__main__":
    main()

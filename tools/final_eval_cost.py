"""Cost of the final evaluation (train.evaluate_with_recon_metrics) at a bench configuration's shape: the forward passes over
`--samples` synthetic test images at the configuration's batch size, with the reconstruction metrics scored in 128-sample
chunks.  Prints one JSON line: wall time of the pass, and the same pass with the metric kernels left out (train.evaluate)
for comparison.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/final_eval_cost.py ...` for per-kernel times
(metric_min_k / metric_ssim_k / metric_finalize_k against the model's kernels).

    python tools/final_eval_cost.py --config C2 --samples 10000
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--samples", type=int, default=10000)
    a = ap.parse_args()
    import bench
    import movae_amd  # noqa: F401
    from movae_amd import train

    cfg = dict(bench.CONFIGS[a.config])
    dev = torch.device("cuda:0")
    net, _, _, args, _ = bench.build_workload(cfg, dev, pool=1)
    args.max_fid_samples = a.samples
    g = torch.Generator().manual_seed(7)
    b = cfg["batch"]
    pool = torch.rand(max(1, 1024 // b) * b, 3, cfg["size"], cfg["size"], generator=g)  # distinct host batches, cycled
    loader = []
    for i in range(0, a.samples, b):
        j = (i // b) % (pool.size(0) // b) * b
        loader.append((pool[j: j + min(b, a.samples - i)], None))
    res = {"config": a.config, "samples": a.samples, "batch": b}
    for name, fn in (("evaluate", lambda: train.evaluate(net, loader, dev, args)),
                     ("evaluate_with_recon_metrics", lambda: train.evaluate_with_recon_metrics(net, loader, dev, args))):
        fn()  # warm-up (library load, allocator)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        res[name + "_s"] = round(time.perf_counter() - t0, 4)
        if isinstance(out, tuple):
            res["recon"] = out[1]
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Ancestral sampling from the PixelCNN priors on one MI355X: the cached sampler (sampling.CachedPixelCNNSampler, one launch per
code, csrc/prior_sample.hip) against full recompute (PixelCNN.sample: one full-grid forward_nhwc, softmax and multinomial per
code), in the same process.  Host clock around work that ends in a device synchronise, after a warm-up of each path; one JSON line.

Shapes (main.py's prior defaults: K 512, D 64, hidden 128, 15 layers):
  C3  the flat prior on 16x16 codes at B = 4 and B = 128
  C4  the hierarchical prior at B = 4: top 32x32 (unconditional), bottom 64x64 (conditioned on the upsampled top embedding)

The cached path is always timed over the whole grid (weight packing included), median of --reps runs.  Every position of the full
path costs the same full-grid forward, so where a grid has more than --full-positions positions the full path is timed over that
many and its total is extrapolated to H*W; the record says so (`full_extrapolated`, `full_positions_timed`).  Before timing, each
shape's teacher-forced cached logits are compared with forward_nhwc of the same codes (`max_abs_logit_diff`).

Usage:  python tools/prior_sample_bench.py [--reps 3] [--full-positions 256] [--only c3|c4]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, D, HIDDEN, LAYERS = 512, 64, 128, 15


def wall_ms(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def full_positions(net, B, H, W, cond, n):
    """The first n raster positions of PixelCNN.sample's loop (models/pixelcnn_prior.py): every position costs the same."""
    import torch

    samples = torch.zeros(B, H, W, dtype=torch.long, device=cond.device if cond is not None else next(net.parameters()).device)
    with torch.no_grad():
        for pos in range(n):
            i, j = divmod(pos, W)
            logits = net.forward_nhwc(samples, cond)[:, i, j, :] / 1.0
            probs = torch.softmax(logits, dim=1)
            samples[:, i, j] = torch.multinomial(probs, 1).squeeze(-1)
    return samples


def level(net, B, H, W, cond_nchw, reps, full_cap):
    """One PixelCNN on one grid: cached over the whole grid, full over min(H*W, full_cap) positions."""
    import torch

    from movae_amd import ops
    from movae_amd.sampling import CachedPixelCNNSampler

    smp = CachedPixelCNNSampler(net)
    cond = ops.to_nhwc(cond_nchw).contiguous() if cond_nchw is not None else None
    z = torch.randint(0, K, (B, H, W), generator=torch.Generator().manual_seed(3)).to(next(net.parameters()).device)
    _, lg = smp.run(B, H, W, condition=cond_nchw, forced=z, return_logits=True)  # (also the cached path's warm-up)
    with torch.no_grad():
        diff = (lg - net.forward_nhwc(z, cond)).abs().max().item()
    cached = [wall_ms(lambda: smp.run(B, H, W, condition=cond_nchw)) for _ in range(reps)]
    n = min(H * W, full_cap)
    full_positions(net, B, H, W, cond, min(n, 4))  # warm-up
    full = wall_ms(lambda: full_positions(net, B, H, W, cond, n)) * (H * W / n)
    return {"B": B, "codes": f"{H}x{W}", "conditional": cond is not None, "launches_cached": H * W, "max_abs_logit_diff": diff,
            "cached_ms": round(statistics.median(cached), 3), "cached_ms_runs": [round(c, 3) for c in cached],
            "cached_us_per_code": round(statistics.median(cached) * 1e3 / (H * W), 2), "full_ms": round(full, 3),
            "full_positions_timed": n, "full_extrapolated": n < H * W, "speedup": round(full / statistics.median(cached), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--full-positions", type=int, default=256, help="positions of the full path timed per grid (the rest extrapolated)")
    ap.add_argument("--only", choices=["c3", "c4"], default=None)
    a = ap.parse_args()

    import torch

    import movae_amd  # noqa: F401
    from movae_amd.models._base import nchw_view
    from movae_amd.models.pixelcnn_prior import HierarchicalPixelCNN, PixelCNN

    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    out = {"tool": "prior_sample_bench", "reps": a.reps, "full_positions": a.full_positions,
           "prior": {"K": K, "D": D, "hidden": HIDDEN, "layers": LAYERS}}
    torch.manual_seed(0)
    if a.only != "c4":
        net = PixelCNN(K, D, HIDDEN, LAYERS).to(dev).eval()
        out["c3"] = [level(net, B, 16, 16, None, a.reps, a.full_positions) for B in (4, 128)]
    if a.only != "c3":
        B = 4
        hier = HierarchicalPixelCNN(K, D, HIDDEN, LAYERS).to(dev).eval()
        z_top = torch.randint(0, K, (B, 32, 32), generator=torch.Generator().manual_seed(4)).to(dev)
        with torch.no_grad():
            cond = nchw_view(hier._condition(z_top))
        top = level(hier.prior_top, B, 32, 32, None, a.reps, a.full_positions)
        bottom = level(hier.prior_bottom, B, 64, 64, cond, a.reps, a.full_positions)
        both = [wall_ms(lambda: hier.sample(B, (32, 32), (64, 64), dev, cached=True)) for _ in range(a.reps)]
        out["c4"] = {"top": top, "bottom": bottom, "cached_sample_ms": round(statistics.median(both), 3),
                     "full_sample_ms_extrapolated": round(top["full_ms"] + bottom["full_ms"], 3),
                     "speedup": round((top["full_ms"] + bottom["full_ms"]) / statistics.median(both), 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

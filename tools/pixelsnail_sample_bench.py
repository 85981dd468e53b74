#!/usr/bin/env python3
"""Ancestral sampling from the PixelSNAIL priors on one MI355X: the K/V-cached sampler (sampling.CachedPixelSNAILSampler, one launch
per code, csrc/prior_sample.hip) against full recompute (PixelSNAIL.sample: one full-grid forward_nhwc, softmax and multinomial per
code), in the same process.  Host clock around work that ends in a device synchronise, after a warm-up of each path; one JSON line.

Shapes (the reference's prior defaults: K 512, D 64, hidden 128, 8 blocks x 2 gated blocks, 8 heads; bottom PixelCNN of 15 layers):
  S3  the flat prior on 16x16 codes at B = 4 and B = 128
  S4  the hierarchical prior at B = 4: the PixelSNAIL top on 32x32, then HierarchicalPixelSNAIL.sample(cached="kv") over 32x32 + 64x64

The cached path is always timed over the whole grid (weight packing included), median of --reps runs.  Every position of the full
path costs the same full-grid forward, so where a grid has more than --full-positions positions the full path is timed over that
many and its total is extrapolated to H*W; the record says so (`full_extrapolated`, `full_positions_timed`).  Before timing, each
shape's teacher-forced cached logits are compared with forward_nhwc of the same codes (`max_abs_logit_diff`, beside `max_abs_logit`:
a freshly initialised 8-block model has logits of order 100), and at S3 B = 4 both with a float64 restatement of the forward.

Usage:  python tools/pixelsnail_sample_bench.py [--reps 3] [--full-positions 128] [--only s3|s4]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from prior_sample_bench import full_positions, wall_ms  # noqa: E402  (the clock and the full path's loop are the PixelCNN tool's)

K, D, HIDDEN, BLOCKS, RES_BLOCKS, HEADS, LAYERS_BOTTOM = 512, 64, 128, 8, 2, 8, 15


def float64_logits(net, z):
    """PixelSNAIL.forward (the reference's pixelcnn_prior.py:95-156, :205-218, eval mode) restated with torch's float64 ops on the
    model's parameters -> NHWC logits.  Only a yardstick for the two fp32 paths: nothing in the package calls it."""
    import math

    import torch
    import torch.nn.functional as F

    def conv(m, x, pad=0, mask=None):
        w = m.weight.detach().double()
        return F.conv2d(x, w if mask is None else w * mask.double(), m.bias.detach().double(), padding=pad)

    B, H, W = z.shape
    L = H * W
    h = torch.cat([net.embedding.weight.detach().double()[z], net._pos_encoding(B, H, W, z.device).double()], -1).permute(0, 3, 1, 2)
    h = conv(net.conv_in, h, net.conv_in.kernel_size // 2, net.conv_in.mask)
    visible = torch.tril(torch.ones(L, L, dtype=torch.bool, device=z.device))
    for blk in net.blocks:
        r = h
        for g in blk.res_blocks:
            o = F.relu(conv(g.conv2, F.relu(conv(g.conv1, r)), 1, g.conv2.mask))
            r = r + torch.sigmoid(conv(g.conv_gate, o)) * torch.tanh(conv(g.conv_feature, o))
        a = blk.attention
        q, k, v = (conv(m, r).view(B, a.num_heads, a.head_dim, L).permute(0, 1, 3, 2) for m in (a.q_proj, a.k_proj, a.v_proj))
        s = (q @ k.transpose(-2, -1) / math.sqrt(a.head_dim)).masked_fill(~visible, float("-inf")).softmax(-1)
        o = (s @ v).permute(0, 3, 1, 2).reshape(B, a.proj_dim, H, W)  # channel d * heads + h
        h = h + (conv(blk.out_conv, torch.cat([r, conv(a.out_proj, o)], 1)) + r)
    return conv(net.conv_out[3], F.relu(conv(net.conv_out[1], F.relu(h)))).permute(0, 2, 3, 1)


def level(net, B, H, W, reps, full_cap, float64=False):
    """One PixelSNAIL on one grid: cached over the whole grid, full over min(H*W, full_cap) positions."""
    import torch

    from movae_amd.sampling import CachedPixelSNAILSampler

    smp = CachedPixelSNAILSampler(net)
    z = torch.randint(0, K, (B, H, W), generator=torch.Generator().manual_seed(3)).to(next(net.parameters()).device)
    _, lg = smp.run(B, H, W, forced=z, return_logits=True)  # (also the cached path's warm-up)
    acc = {}
    with torch.no_grad():
        fw = net.forward_nhwc(z)
        diff = (lg - fw).abs().max().item()
        if float64:  # which of the two fp32 paths is nearer the exact logits
            ref = float64_logits(net, z)
            acc = {"max_abs_cached_minus_float64": (lg.double() - ref).abs().max().item(),
                   "max_abs_forward_minus_float64": (fw.double() - ref).abs().max().item()}
    cached = [wall_ms(lambda: smp.run(B, H, W)) for _ in range(reps)]
    n = min(H * W, full_cap)
    full_positions(net, B, H, W, None, min(n, 2))  # warm-up
    full = wall_ms(lambda: full_positions(net, B, H, W, None, n)) * (H * W / n)
    d = smp.dims()
    return {"B": B, "codes": f"{H}x{W}", "launches_cached": H * W, "max_abs_logit_diff": diff, "max_abs_logit": fw.abs().max().item(), **acc,
            "packed_weight_bytes": 4 * smp.pack_weights().numel(), "kv_bytes_per_sample_at_last_code": 4 * H * W * d[3] * 2 * d[5] * d[6],
            "cached_ms": round(statistics.median(cached), 3), "cached_ms_runs": [round(c, 3) for c in cached],
            "cached_us_per_code": round(statistics.median(cached) * 1e3 / (H * W), 2), "full_ms": round(full, 3),
            "full_positions_timed": n, "full_extrapolated": n < H * W, "speedup": round(full / statistics.median(cached), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--full-positions", type=int, default=128, help="positions of the full path timed per grid (the rest extrapolated)")
    ap.add_argument("--only", choices=["s3", "s4"], default=None)
    a = ap.parse_args()

    import torch

    import movae_amd  # noqa: F401
    from movae_amd import ops
    from movae_amd.models._base import nchw_view
    from movae_amd.models.pixelcnn_prior import HierarchicalPixelSNAIL, PixelSNAIL

    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    out = {"tool": "pixelsnail_sample_bench", "reps": a.reps, "full_positions": a.full_positions,
           "prior": {"K": K, "D": D, "hidden": HIDDEN, "blocks": BLOCKS, "res_blocks": RES_BLOCKS, "heads": HEADS,
                     "layers_bottom": LAYERS_BOTTOM}}
    torch.manual_seed(0)
    if a.only != "s4":
        net = PixelSNAIL(K, D, HIDDEN, num_blocks=BLOCKS, num_res_blocks_per_layer=RES_BLOCKS, num_heads=HEADS).to(dev).eval()
        out["s3"] = [level(net, B, 16, 16, a.reps, a.full_positions, float64=B == 4) for B in (4, 128)]
    if a.only != "s3":
        B = 4
        hier = HierarchicalPixelSNAIL(K, D, HIDDEN, num_blocks_top=BLOCKS, num_res_blocks_per_layer=RES_BLOCKS, num_heads=HEADS,
                                      num_layers_bottom=LAYERS_BOTTOM).to(dev).eval()
        top = level(hier.prior_top, B, 32, 32, a.reps, a.full_positions)
        # the PixelCNN bottom of the same model: cached (what cached=True already gave) and full, for the totals below
        z_top = torch.randint(0, K, (B, 32, 32), generator=torch.Generator().manual_seed(4)).to(dev)
        with torch.no_grad():
            cond = nchw_view(hier._condition(z_top))
        bot = hier.prior_bottom.cached_sampler()
        bot.run(B, 64, 64, condition=cond)
        bottom_cached = statistics.median([wall_ms(lambda: bot.run(B, 64, 64, condition=cond)) for _ in range(a.reps)])
        cond_nhwc = ops.to_nhwc(cond).contiguous()
        n = min(64 * 64, a.full_positions)
        full_positions(hier.prior_bottom, B, 64, 64, cond_nhwc, 2)
        bottom_full = wall_ms(lambda: full_positions(hier.prior_bottom, B, 64, 64, cond_nhwc, n)) * (64 * 64 / n)
        both = [wall_ms(lambda: hier.sample(B, (32, 32), (64, 64), dev, cached="kv")) for _ in range(a.reps)]
        kv = statistics.median(both)
        out["s4"] = {"top": top, "bottom_cached_ms": round(bottom_cached, 3), "bottom_full_ms_extrapolated": round(bottom_full, 3),
                     "bottom_full_positions_timed": n, "cached_kv_sample_ms": round(kv, 3),
                     "cached_kv_sample_ms_runs": [round(c, 3) for c in both],
                     "cached_true_sample_ms_extrapolated": round(top["full_ms"] + bottom_cached, 3),
                     "full_sample_ms_extrapolated": round(top["full_ms"] + bottom_full, 3),
                     "speedup_over_cached_true": round((top["full_ms"] + bottom_cached) / kv, 2),
                     "speedup_over_full": round((top["full_ms"] + bottom_full) / kv, 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

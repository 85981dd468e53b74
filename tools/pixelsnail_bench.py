#!/usr/bin/env python3
"""PixelSNAIL cost on one MI355X: the fused causal attention (csrc/attention.hip) against the torch-on-ROCm composition of the
reference's expression (models/pixelcnn_prior.py:118-131: matmul, masked_fill, softmax, dropout, matmul -- a yardstick inside this
tool only), and one prior training step next to the PixelCNN step at the same shapes.  Device events after warm-up; one JSON line.

Attention: forward + backward with dropout 0.1 (training mode), B=128 heads=8 hd=16 at L in {64, 256, 1024} and B=16 at L=4096.
FLOP counts the causal half of the six products a forward + backward needs (QK^T, PV; dP, dV, dQ, dK); bytes count one read of
every input and one write of every output of the fused form; `floor_ms` is the larger of FLOP / 157.3 TFLOP/s (fp32 MFMA peak) and
bytes / 8 TB/s (HBM), `frac_of_floor` = floor / measured.

Prior step: main.py's defaults (K 512, D 64, hidden 128; PixelSNAIL 8 blocks x 2 residual blocks, 8 heads, dropout 0.1; PixelCNN
15 layers) -- zero_grad, loss, backward, clip_grad_norm_(1.0), FusedAdam -- on 8x8 codes at B=128 and 32x32 codes at B=32.

Usage:  python tools/pixelsnail_bench.py [--steps 20] [--warmup 5] [--prior-step-only] [--attention-only] [--dtype fp32|bf16]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FLOPS, HBM_BPS = 157.3e12, 8.0e12
ATTN = [(128, 8, 16, 64), (128, 8, 16, 256), (128, 8, 16, 1024), (16, 8, 16, 4096)]
PRIOR = [(128, 8), (32, 32)]


def timed(fn, steps, warmup):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def torch_reference(q, k, v, heads, p):
    """The reference's expression on [B, proj, L] projections (the NCHW conv outputs, flattened)."""
    import torch
    import torch.nn.functional as F

    B, proj, n = q.shape
    hd = proj // heads
    qh, kh, vh = (t.view(B, heads, hd, n).permute(0, 1, 3, 2) for t in (q, k, v))
    attn = torch.matmul(qh, kh.transpose(-2, -1)) / math.sqrt(hd)
    mask = torch.tril(torch.ones(n, n, device=q.device)).unsqueeze(0)
    attn = attn.masked_fill(mask.unsqueeze(1) == 0, float("-inf"))
    attn = F.dropout(F.softmax(attn, dim=-1), p, training=True)
    out = torch.matmul(attn, vh)
    return out.permute(0, 2, 3, 1).reshape(B, n, proj)


def attention_case(B, heads, hd, n, p, steps, warmup):
    import torch

    from movae_amd import ops

    dev = torch.device("cuda:0")
    proj = heads * hd
    g = torch.Generator(device=dev).manual_seed(0)
    q, k, v, do = (torch.randn(B, n, proj, device=dev, generator=g) for _ in range(4))
    q.requires_grad_(True), k.requires_grad_(True), v.requires_grad_(True)
    draw = [0]

    def fused():
        draw[0] += 1
        o = ops.causal_attention(q, k, v, heads, p, 1234, draw[0])
        torch.autograd.backward(o, do)

    pairs = B * heads * n * (n + 1) / 2
    flop = 6 * 2 * pairs * hd
    nbytes = (4 + 8) * B * n * proj * 4
    floor_ms = max(flop / PEAK_FLOPS, nbytes / HBM_BPS) * 1e3
    rec = {"B": B, "heads": heads, "hd": hd, "L": n, "gflop": round(flop / 1e9, 3), "mbytes": round(nbytes / 1e6, 3),
           "floor_ms": round(floor_ms, 5), "floor": "mfma" if flop / PEAK_FLOPS > nbytes / HBM_BPS else "hbm"}
    ms = timed(fused, steps, warmup)
    rec.update(fused_ms=round(ms, 4), fused_frac_of_floor=round(floor_ms / ms, 4))
    # the composition reads the projections as the reference does: [B, proj, L] (its NCHW conv outputs)
    qt, kt, vt = (t.detach().transpose(1, 2).contiguous().requires_grad_(True) for t in (q, k, v))

    def composed():
        o = torch_reference(qt, kt, vt, heads, p)
        torch.autograd.backward(o, do)

    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    try:
        ms_t = timed(composed, max(1, steps // 2), 1)
        rec.update(torch_ms=round(ms_t, 4), torch_frac_of_floor=round(floor_ms / ms_t, 4), speedup=round(ms_t / ms, 2),
                   torch_peak_gb=round((torch.cuda.max_memory_allocated() - base) / 1e9, 2))
    except torch.cuda.OutOfMemoryError:
        rec.update(torch_ms=None, torch_oom=True)
    qt = kt = vt = None
    torch.cuda.empty_cache()
    return rec


def prior_step_case(kind, B, s, steps, warmup):
    import torch

    from movae_amd.models import PixelCNN, PixelSNAIL
    from movae_amd.optim import FusedAdam, clip_grad_norm_

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    K = 512
    if kind == "pixelsnail":
        net = PixelSNAIL(K, 64, 128, num_blocks=8, num_res_blocks_per_layer=2, num_heads=8, dropout=0.1)
    else:
        net = PixelCNN(K, 64, 128, num_layers=15)
    net = net.to(dev).train()
    opt = FusedAdam(net.parameters(), lr=3e-4, weight_decay=0.0)
    z = torch.randint(0, K, (B, s, s), generator=torch.Generator().manual_seed(1)).to(dev)

    def step():
        opt.zero_grad()
        loss = net.loss(z)
        loss.backward()
        clip_grad_norm_(net.parameters(), max_norm=1.0)
        opt.step()

    return round(timed(step, steps, warmup), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--prior-step-only", action="store_true", help="only the PixelSNAIL prior steps (for a profiler run)")
    ap.add_argument("--attention-only", action="store_true", help="only the attention rows")
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="fp32",
                    help="compute dtype of the fused attention rows and the prior steps (movae_set_compute_dtype); the torch side and "
                         "the floor (fp32 MFMA peak) stay as they are")
    a = ap.parse_args()

    import torch

    import movae_amd  # noqa: F401
    from movae_amd import _lib as L

    assert torch.cuda.is_available(), "needs an MI355X"
    L.set_compute_dtype(a.dtype)
    out = {"tool": "pixelsnail_bench", "steps": a.steps, "warmup": a.warmup, "dtype": a.dtype}
    if not a.prior_step_only:
        out["attention"] = [attention_case(B, h, hd, n, 0.1, a.steps, a.warmup) for B, h, hd, n in ATTN]
    out["prior_step"] = []
    for B, s in ([] if a.attention_only else PRIOR):
        rec = {"B": B, "codes": f"{s}x{s}", "pixelsnail_ms": prior_step_case("pixelsnail", B, s, a.steps, a.warmup)}
        if not a.prior_step_only:
            rec["pixelcnn_ms"] = prior_step_case("pixelcnn", B, s, a.steps, a.warmup)
        out["prior_step"].append(rec)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

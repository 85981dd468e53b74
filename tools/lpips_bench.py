#!/usr/bin/env python3
"""Cost of the final evaluation's LPIPS per 128-sample chunk: 128 x 3 x 32 x 32 and 128 x 3 x 64 x 64 image pairs, the real VGG16
widths up to relu4_3 (default-init weights: the arithmetic does not depend on the values), fp32.

Per shape: the time of metrics.lpips_into per chunk; its split into the feature stack (perceptual.LpipsFeatures on the 2 x 128
normalised images) and the distance part (four movae_lpips_layer + one movae_lpips_finalize, metrics.feature_distance_into); each
distance launch alone, as achieved bytes/s against the 2 * 4 * n * h * w * c bytes it has to read; and, as the baseline of the distance
part, the torch composition of the reference's expression (F.normalize x 2, subtract, square, sum, mean; utils/metrics.py:334-355) on
the same device and the same four feature pairs (as NCHW views of the NHWC buffers and as contiguous NCHW copies, which is what the
reference holds).  Medians of --repeats windows, the two sides alternating.  Prints one JSON line.  bench.py is not touched.

Usage:  python tools/lpips_bench.py [--iters 20] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=128)
    a = ap.parse_args()

    import torch
    import torch.nn.functional as F

    import movae_amd  # noqa: F401
    from movae_amd import _lib as L
    from movae_amd import metrics, perceptual

    dev = torch.device("cuda:0")
    n = a.chunk
    torch.manual_seed(0)
    perceptual.use_vgg16_weights(perceptual._default_init(perceptual.LPIPS_VGG16_WIDTHS))
    res = {"chunk": n, "widths": list(perceptual.LPIPS_VGG16_WIDTHS), "dtype": "fp32"}

    def window(fn, iters):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / iters * 1e3  # us per call, eager launches

    def timed(fns, iters):
        """medians (us) and [min, max] of the callables, warmed up, their windows alternating"""
        for fn in fns:
            window(fn, 3)
        ts = [[] for _ in fns]
        for _ in range(a.repeats):
            for t, fn in zip(ts, fns):
                t.append(window(fn, iters))
        return [statistics.median(t) for t in ts], [[min(t), max(t)] for t in ts]

    for side in (32, 64):
        g = torch.Generator().manual_seed(side)
        real = torch.rand(n, 3, side, side, generator=g).to(dev)
        recon = torch.tanh(torch.randn(n, side, side, 3, generator=g)).to(dev).permute(0, 3, 1, 2)  # the decoder's NHWC buffer
        out = torch.empty(1 + n, dtype=torch.float32, device=dev)
        feats = metrics._features_on(dev, perceptual.registered_vgg16_lpips_weights())
        both = torch.cat([real.permute(0, 2, 3, 1), recon.permute(0, 2, 3, 1)]).contiguous()
        taps = feats(both)
        pairs = [(f[:n], f[n:]) for f in taps]
        views = [(p.permute(0, 3, 1, 2), q.permute(0, 3, 1, 2)) for p, q in pairs]
        copies = [(p.contiguous(), q.contiguous()) for p, q in views]

        def torch_distance(ps):
            scores = []
            for f1, f2 in ps:
                b, c = f1.shape[:2]
                d = (F.normalize(f1.reshape(b, c, -1), p=2, dim=1) - F.normalize(f2.reshape(b, c, -1), p=2, dim=1)) ** 2
                scores.append(d.sum(dim=1).mean(dim=1))
            return torch.stack(scores, dim=0).mean(dim=0).mean()

        tag = f"{side}x{side}"
        (t_all, t_feat, t_dist, t_tv, t_tc), spread = timed(
            [lambda: metrics.lpips_into(out, real, recon), lambda: feats(both), lambda: metrics.feature_distance_into(out, pairs),
             lambda: torch_distance(views), lambda: torch_distance(copies)], a.iters)
        res[f"{tag}_lpips_into_us"], res[f"{tag}_feature_stack_us"], res[f"{tag}_distance_hip_us"] = t_all, t_feat, t_dist
        res[f"{tag}_distance_torch_nhwc_views_us"], res[f"{tag}_distance_torch_nchw_us"] = t_tv, t_tc
        res[f"{tag}_spread_us"] = spread
        want = float(torch_distance([(p.double(), q.double()) for p, q in copies]).item())
        res[f"{tag}_value_hip"], res[f"{tag}_value_torch_f64"] = float(metrics.feature_distance_into(out, pairs)[0].item()), want
        # each distance launch alone
        lib = L.load()
        st = L.stream_ptr(dev)
        for (f1, f2), name in zip(pairs, ("relu1_2", "relu2_2", "relu3_3", "relu4_3")):
            nbytes = lib.movae_lpips_ws_bytes(*f1.shape)
            part = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
            (us,), _ = timed([lambda: L.call("movae_lpips_layer", f1.data_ptr(), f2.data_ptr(), *f1.shape, 1.0, part.data_ptr(), nbytes, st)],
                             5 * a.iters)
            moved = 2 * 4 * f1.numel()
            res[f"{tag}_{name}"] = {"shape": list(f1.shape), "us": us, "bytes": moved, "GBps": moved / (us * 1e-6) / 1e9}
    perceptual.use_vgg16_weights(None)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

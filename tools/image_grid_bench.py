#!/usr/bin/env python3
"""Cost of one image grid: visual.image_grid (movae_image_grid_u8: one launch pair, float batch -> uint8 picture) against the plain-torch
composition of make_grid and save_image's quantisation (amin / amax, clamp, normalise, pad and place, permute, * 255 + 0.5, clamp, byte
cast) on the same device in the same process, in the mode every figure uses (normalize=True over the batch's own range).

Shapes: 16 x 3 x 32 x 32 (nrow 4), 64 x 3 x 64 x 64 (nrow 8) and 100 x 3 x 256 x 256 (nrow 10), seeded values in [-1, 1).  Each side is
warmed up, then timed with device events over windows of --iters calls; the two sides alternate and the median of --repeats windows is
reported with the spread.  The two pictures are compared byte for byte (the torch side divides, like the kernel).  The device-to-host
copy of the picture, the same on both sides, is timed on its own.  Prints one JSON line.  bench.py is not touched.

Usage:  python tools/image_grid_bench.py [--repeats 7] [--iters 50]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [((16, 3, 32, 32), 4), ((64, 3, 64, 64), 8), ((100, 3, 256, 256), 10)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()

    import torch

    import movae_amd  # noqa: F401
    from movae_amd import visual

    if not torch.cuda.is_available():
        raise SystemExit("image_grid_bench needs an MI355X: a CPU run gives no time")
    dev = torch.device("cuda:0")
    padding = 2

    def torch_grid(x, nrow):
        n, c, h, w = x.shape
        lo, hi = x.amin(), x.amax()
        v = (x.clamp(lo, hi) - lo) / (hi - lo).clamp_min(1e-5)
        xmaps = min(nrow, n)
        ymaps = -(-n // xmaps)
        grid = torch.zeros((c, ymaps * (h + padding) + padding, xmaps * (w + padding) + padding), device=x.device)
        k = 0
        for y in range(ymaps):
            for xx in range(xmaps):
                if k >= n:
                    break
                grid[:, y * (h + padding) + padding: y * (h + padding) + padding + h,
                     xx * (w + padding) + padding: xx * (w + padding) + padding + w] = v[k]
                k += 1
        return grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8)

    def window(fn, iters):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / iters

    res = {"mode": "minmax", "padding": padding, "iters": a.iters, "repeats": a.repeats, "shapes": []}
    with torch.no_grad():
        for shape, nrow in SHAPES:
            x = (torch.rand(shape, generator=torch.Generator().manual_seed(0)) * 2 - 1).to(dev)
            hip = lambda: visual.image_grid(x, nrow=nrow, padding=padding, normalize=True)  # noqa: E731
            ref = lambda: torch_grid(x, nrow)  # noqa: E731
            got, want = hip(), ref()  # (the warm-up; also what is compared)
            torch.cuda.synchronize()
            rec = {"shape": list(shape), "nrow": nrow, "picture": list(got.shape), "bytes_differing": int((got != want).sum().item())}
            ts = ([], [])
            for _ in range(a.repeats):
                for t, fn in zip(ts, (hip, ref)):
                    t.append(window(fn, a.iters))
            rec["hip_ms"], rec["torch_ms"] = statistics.median(ts[0]), statistics.median(ts[1])
            rec["hip_spread_ms"], rec["torch_spread_ms"] = [min(ts[0]), max(ts[0])], [min(ts[1]), max(ts[1])]
            # the least traffic: every float read once (twice in this mode: the range pass), every byte written once
            rec["min_bytes"] = 2 * x.numel() * 4 + got.numel()
            rec["hip_gbps"] = rec["min_bytes"] / (rec["hip_ms"] * 1e-3) / 1e9
            rec["d2h_ms"] = statistics.median(window(lambda: got.cpu(), 5) for _ in range(3))
            print(f"{shape}: hip {rec['hip_ms']:.4f} ms, torch {rec['torch_ms']:.4f} ms, {rec['bytes_differing']} bytes differ",
                  file=sys.stderr, flush=True)
            res["shapes"].append(rec)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

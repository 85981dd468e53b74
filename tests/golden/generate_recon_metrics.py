#!/usr/bin/env python3
"""Golden vectors of the reconstruction metrics (runs ONLY in the build container, never on the GPU box).

Imports the reference's utils/metrics.py (ssim, psnr, ssnr) by path and records their results on the cases below into
recon_metrics.npz next to this script (plain arrays, no pickle; inputs + expected outputs only, no reference source text).
utils/metrics.py imports torchvision at module level for its Inception / VGG feature extractors; torchvision is not installed
here and ssim / psnr / ssnr never touch it, so empty placeholder modules stand in for it.

The chunked numbers of main.py:335-373 (_compute_recon_metrics_from_tensors: the reference's ssim / psnr per 128-sample
chunk, unweighted means over the chunks) are recorded for a 300-sample collection (chunks 128 + 128 + 44) built from a seed
by `collection()`; main.py itself cannot be imported without its training dependencies, so the chunk loop is restated here in
its three lines (slice, score, np.mean).  The largest case (256 x 256) is stored as its seed as well: `case_images()` rebuilds it.

Usage:  python tests/golden/generate_recon_metrics.py        (seconds; writes recon_metrics.npz bit for bit the same each run)
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("MOVAE_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "recon_metrics.npz")

#: (name, batch, channels, side, kind, window_size, stored); stored False: rebuilt from the seed by case_images()
CASES = [
    ("u01_32", 2, 3, 32, "u01", 11, True),
    ("pm1_32", 2, 3, 32, "pm1", 11, True),
    ("mixed_28", 5, 3, 28, "mixed", 11, True),
    ("u01_8", 1, 1, 8, "u01", 11, True),
    ("pm1_40_w7", 5, 1, 40, "pm1", 7, True),
    ("outside_64", 2, 3, 64, "outside", 11, True),
    ("identical_32", 3, 3, 32, "identical", 11, True),
    ("constant_32", 2, 1, 32, "constant", 11, True),
    ("mixed_64_w7", 1, 3, 64, "mixed", 7, True),
    ("u01_40", 1, 3, 40, "u01", 11, True),
    ("pm1_8_w7", 2, 3, 8, "pm1", 7, True),
    ("close_32", 5, 3, 32, "close", 11, True),
    ("mixed_256", 1, 3, 256, "mixed", 11, False),
]
COLLECTION = dict(n=300, c=3, side=32, seed=300)


def case_images(i):
    """(real, recon) float32 NCHW of case i, from a CPU generator seeded by the case index."""
    _, b, c, s, kind, _, _ = CASES[i]
    g = torch.Generator().manual_seed(1000 + i)
    u = torch.rand(b, c, s, s, generator=g)
    v = torch.rand(b, c, s, s, generator=g)
    if kind == "u01":
        return u, v
    if kind == "pm1":
        return 2 * u - 1, 2 * v - 1
    if kind == "mixed":  # real in [0, 1], recon from a tanh output layer
        return u, torch.tanh(3 * (2 * v - 1))
    if kind == "outside":  # both leave the range: the clamps act on each side
        return 3.5 * u - 1.5, 2.5 * v - 0.5
    if kind == "identical":
        return u, u.clone()
    if kind == "constant":
        return torch.full_like(u, 0.3), torch.full_like(v, 0.7)
    if kind == "close":  # a good reconstruction: high SSIM / PSNR
        return u, (u + 0.02 * (2 * v - 1)).clamp(0, 1)
    raise ValueError(kind)


def collection():
    """300 (real, recon) pairs of 3 x 32 x 32 whose [-1, 1] decisions differ per 128-sample chunk: real is negative only in
    samples 250..255 (the end of chunk 1), recon only in samples 0..5 and 128..130 (the starts of chunks 0 and 1)."""
    d = COLLECTION
    g = torch.Generator().manual_seed(d["seed"])
    real = torch.rand(d["n"], d["c"], d["side"], d["side"], generator=g)
    recon = (real + 0.1 * torch.randn(real.shape, generator=g)).clamp(0, 1)
    real[250:256] = 2 * real[250:256] - 1
    recon[0:6] = 2 * recon[0:6] - 1
    recon[128:131] = 2 * recon[128:131] - 1
    return real, recon


def _reference_metrics():
    for name in ("torchvision", "torchvision.models", "torchvision.transforms"):
        sys.modules.setdefault(name, types.ModuleType(name))
    tvm = sys.modules["torchvision.models"]
    for attr in ("inception_v3", "Inception_V3_Weights", "vgg16", "VGG16_Weights"):
        setattr(tvm, attr, None)
    sys.modules["torchvision.transforms"].functional = types.ModuleType("torchvision.transforms.functional")
    sys.modules["torchvision"].models = tvm
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    spec = importlib.util.spec_from_file_location("_ref_metrics", os.path.join(REF, "utils", "metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    torch.set_num_threads(1)  # one summation order for the CPU convolutions and reductions
    M = _reference_metrics()
    out = {}
    names = []
    for i, (name, b, c, s, kind, ws, stored) in enumerate(CASES):
        real, recon = case_images(i)
        names.append(name)
        out[f"{name}.shape"] = np.array([b, c, s, s], dtype=np.int64)
        out[f"{name}.window"] = np.array(ws, dtype=np.int64)
        out[f"{name}.index"] = np.array(i, dtype=np.int64)
        if stored:
            out[f"{name}.real"] = real.numpy()
            out[f"{name}.recon"] = recon.numpy()
        with torch.no_grad():
            out[f"{name}.ssim"] = np.array(M.ssim(real, recon, window_size=ws, size_average=True).item(), dtype=np.float64)
            out[f"{name}.ssim_per_image"] = M.ssim(real, recon, window_size=ws, size_average=False).numpy().astype(np.float64)
            out[f"{name}.psnr"] = np.array(M.psnr(real, recon), dtype=np.float64)
            out[f"{name}.ssnr"] = np.array(M.ssnr(real, recon), dtype=np.float64)
    out["cases"] = np.array(names)
    real, recon = collection()
    ssim_vals, psnr_vals = [], []
    with torch.no_grad():
        for i in range(0, real.size(0), 128):
            ssim_vals.append(M.ssim(real[i:i + 128], recon[i:i + 128], size_average=True).item())
            psnr_vals.append(M.psnr(real[i:i + 128], recon[i:i + 128]))
    out["collection.chunk_ssim"] = np.array(ssim_vals, dtype=np.float64)
    out["collection.chunk_psnr"] = np.array(psnr_vals, dtype=np.float64)
    out["collection.ssim"] = np.array(np.mean(ssim_vals), dtype=np.float64)
    out["collection.psnr"] = np.array(np.mean(psnr_vals), dtype=np.float64)
    np.savez(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Golden vectors of the final evaluation's LPIPS (runs ONLY in the build container, on the CPU, never on the GPU box).

Imports the reference's utils/metrics.py by path, in the manner of generate_recon_metrics.py (whose placeholder torchvision modules
this reuses), and lets the reference's own VGGFeatureExtractor.__init__, its forward hooks and lpips() run unmodified.  torchvision is
bypassed: the two names the module took from it, `vgg16` and `VGG16_Weights`, are replaced in the imported module's namespace, and
`vgg16(...)` returns an object whose `.features` is a seeded Sequential of the full VGG16 topology (13 convolutions with ReLU, 5 pools:
31 entries) with the narrow widths below and Kaiming-normal weights (torchvision's VGG init: features of order one).

  lpips_tiny.npz   the twenty tensors of conv1_1 .. conv4_3 (`vgg.features.N.*`; the conv5 block the reference runs and discards is
                   not recorded), and for each case below the image pairs and the reference's lpips() in fp32 and, from a .double()
                   copy of the extractor on the same images, in fp64.

Cases (B x C x H x W) and variants: `a` real in [0, 1], recon with negatives; `b` the reverse; `same` identical operands.  The
32 x 32 cases pair independent images (a large distance); the 40 x 36 case (non-square, odd pooled sizes 20 x 18 -> 10 x 9 -> 5 x 4)
pairs an image with a noisy copy of itself in the other range (the small distance of a good reconstruction).

Usage:  python tests/golden/generate_lpips.py        (seconds)
"""
import importlib.util
import os
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "lpips_tiny.npz")

#: conv1_1 .. conv4_3, then the conv5 block (run by the reference, tapped by nothing)
WIDTHS = (8, 8, 16, 16, 32, 32, 32, 64, 64, 64, 64, 64, 64)
POOL_AFTER = (1, 3, 6, 9, 12)  # (0-based convolution number) torchvision's cfg "D"
RECORDED = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21)  # torchvision's indices of the ten convolutions up to conv4_3
STACK_SEED = 5151
CASES = (("3x3x32x32", (3, 3, 32, 32), "independent"), ("2x3x40x36", (2, 3, 40, 36), "close"), ("2x1x32x32", (2, 1, 32, 32), "independent"))
VARIANTS = ("a", "b", "same")


def narrow_vgg16(*_args, **_kwargs):
    """Stands in for torchvision.models.vgg16: the same weights at every call."""
    state = torch.get_rng_state()
    torch.manual_seed(STACK_SEED)
    layers, cin = [], 3
    for i, co in enumerate(WIDTHS):
        conv = nn.Conv2d(cin, co, 3, padding=1)
        nn.init.kaiming_normal_(conv.weight, mode="fan_out", nonlinearity="relu")
        nn.init.uniform_(conv.bias, -0.1, 0.1)
        layers += [conv, nn.ReLU(inplace=True)]
        if i in POOL_AFTER:
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        cin = co
    torch.set_rng_state(state)
    net = nn.Module()
    net.features = nn.Sequential(*layers)
    assert len(net.features) == 31
    return net


def case_pairs(index):
    """{variant: (real, recon)} float32 NCHW of case `index`, from a CPU generator seeded by it."""
    _, shape, kind = CASES[index]
    g = torch.Generator().manual_seed(STACK_SEED + 1 + index)
    unit = lambda: torch.rand(shape, generator=g) * 0.96 + 0.02  # noqa: E731  (off the clamp edges)
    pairs = {}
    for v in ("a", "b"):
        u = unit()
        if kind == "close":
            s = (2 * u - 1 + 0.05 * torch.randn(shape, generator=g)).clamp(-0.98, 0.98)
        else:
            s = torch.rand(shape, generator=g) * 1.96 - 0.98
        pairs[v] = (u, s) if v == "a" else (s, u)
    pairs["same"] = (pairs["a"][0], pairs["a"][0].clone())
    return pairs


def _reference_metrics():
    spec = importlib.util.spec_from_file_location("_gen_recon_metrics", os.path.join(HERE, "generate_recon_metrics.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    M = gen._reference_metrics()
    M.vgg16 = narrow_vgg16
    M.VGG16_Weights = types.SimpleNamespace(DEFAULT=None)
    return M


def main():
    torch.set_num_threads(1)  # one summation order for the CPU convolutions and reductions
    M = _reference_metrics()
    out = {}
    sd = narrow_vgg16().features.state_dict()
    for n in RECORDED:
        for leaf in ("weight", "bias"):
            out[f"vgg.features.{n}.{leaf}"] = sd[f"{n}.{leaf}"].numpy().copy()
    names = []
    for i, (tag, shape, _) in enumerate(CASES):
        for v, (real, recon) in case_pairs(i).items():
            name = f"{tag}.{v}"
            names.append(name)
            assert (real.min() < 0, recon.min() < 0) == {"a": (False, True), "b": (True, False), "same": (False, False)}[v]
            if v != "same":
                out[f"{name}.real"], out[f"{name}.recon"] = real.numpy(), recon.numpy()
            for prec, dtype in (("f32", torch.float32), ("f64", torch.float64)):
                if hasattr(M.lpips, "_feature_extractor"):
                    del M.lpips._feature_extractor  # (the reference caches its extractor on the function)
                if dtype == torch.float64:
                    M.lpips._feature_extractor = M.VGGFeatureExtractor(device="cpu").double()
                assert len(M.VGGFeatureExtractor(device="cpu").features) == 30
                out[f"{name}.lpips.{prec}"] = np.array(M.lpips(real.to(dtype), recon.to(dtype), device="cpu"), dtype=np.float64)
            print(f"{name}: lpips {float(out[f'{name}.lpips.f64']):.8f}, fp32 deviation "
                  f"{abs(float(out[f'{name}.lpips.f32']) - float(out[f'{name}.lpips.f64'])):.2e}")
    del M.lpips._feature_extractor
    out["cases"] = np.array(names)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} keys={len(out)} bytes={os.path.getsize(OUT)}")


if __name__ == "__main__":
    main()

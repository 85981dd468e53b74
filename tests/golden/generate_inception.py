#!/usr/bin/env python3
"""Golden vectors of the final evaluation's rFID (runs ONLY in the build container, on the CPU, never on the GPU box).

Imports the reference's utils/metrics.py by path and lets its own calculate_fid / extract_inception_features / fid_from_features /
InceptionV3.forward run unmodified.  torchvision is not installed: a stub is put into sys.modules whose `models.inception_v3` returns
the plain-torch module below -- the Inception-v3 topology with torchvision's attribute names at 1/8 of the real widths (feature
dimension 256), seeded weights and non-trivial BatchNorm running statistics -- and whose `transforms.functional` resize / center_crop
/ normalize are restated on F.interpolate(mode="bicubic", antialias=True).  THE TOPOLOGY IS WRITTEN FROM KNOWLEDGE of torchvision's
public definition, not copied from or compared with it.

  inception_tiny.npz
    sd.<key>                 the module's state_dict.  Convolution weights are stored as float16: they were rounded to float16 BEFORE
                             every run here, so the float32 weights the runs used are exactly these values (a float32 copy of the
                             0.37 M parameters would exceed the size limit of a committed file).
    stack.<tag>.{seed,shape} inputs of the bare stack (NORMALISED images, standard normal from the seed), 75 x 75 (Mixed_7 at 1 x 1),
    stack.<tag>.{f32,f64}    83 x 91 and 299 x 299, and the reference InceptionV3.forward's features in float32 and float64.
    feat.<tag>.{seed,shape}  raw images (see `raw_images`) and extract_inception_features' result, float32 and float64.
    feat.<tag>.{f32,f64}
    fid.{seed,n,side}        two sets of N = 320 > D images at 32 x 32 (see `fid_sets`)
    fid.ref                  calculate_fid(real, fake) of the reference, float32 CPU
    fid.f64                  the same from a float64 copy of the module on float64 images
    fid.f32_cl               the same from a second float32 run in channels_last memory (another accumulation order)
    fid.features             [2, 320, 48] float32: the first 48 feature dimensions of both sets (N > D), for the CPU test of
    fid.from_features        fid_from_features, and the reference's fid_from_features on exactly these values (as float64)
    fid.yardstick            max |fp32 run - fid.f64| over the two fp32 runs: the error a correct fp32 implementation makes
    fid.no_antialias, fid.no_denorm    FID with the resize replaced by the plain a = -0.75 bicubic / without the 0.5 x + 0.5 step

Asserted here: yardstick < 1e-3 of the FID, and both wrong pipelines differ from fid.ref by more than 10 times the GPU test's bound
(4 x yardstick) -- the test can fail.

Usage:  python tests/golden/generate_inception.py        (about a minute)
"""
import enum
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("MOVAE_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "inception_tiny.npz")
SEED = 2929
DIV = 8  # every width of the real network divides by 8
STACK_CASES = (("75x75", (3, 3, 75, 75)), ("83x91", (2, 3, 83, 91)), ("299x299", (2, 3, 299, 299)))
FEAT_CASES = (("32x32", (5, 3, 32, 32)), ("40x64", (2, 3, 40, 64)))
FID_N, FID_SIDE = 320, 32

#: what the stub's inception_v3 hands out: dtype and memory format of the module (switched between the runs below)
MODE = {"dtype": torch.float32, "channels_last": False, "resize": "antialias"}


# ---- the narrow network -----------------------------------------------------------------------------------------------
class BasicConv2d(nn.Module):
    def __init__(self, cin, cout, **kw):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, bias=False, **kw)
        self.bn = nn.BatchNorm2d(cout, eps=0.001)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)))


def _w(c):
    return c // DIV


class BlockA(nn.Module):
    def __init__(self, cin, pool):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, _w(64), kernel_size=1)
        self.branch5x5_1 = BasicConv2d(cin, _w(48), kernel_size=1)
        self.branch5x5_2 = BasicConv2d(_w(48), _w(64), kernel_size=5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, _w(64), kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(_w(64), _w(96), kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(_w(96), _w(96), kernel_size=3, padding=1)
        self.branch_pool = BasicConv2d(cin, _w(pool), kernel_size=1)

    def forward(self, x):
        a = self.branch1x1(x)
        b = self.branch5x5_2(self.branch5x5_1(x))
        c = self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x)))
        d = self.branch_pool(F.avg_pool2d(x, kernel_size=3, stride=1, padding=1))
        return torch.cat([a, b, c, d], 1)


class BlockB(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3 = BasicConv2d(cin, _w(384), kernel_size=3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, _w(64), kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(_w(64), _w(96), kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(_w(96), _w(96), kernel_size=3, stride=2)

    def forward(self, x):
        a = self.branch3x3(x)
        b = self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x)))
        return torch.cat([a, b, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


class BlockC(nn.Module):
    def __init__(self, cin, c7):
        super().__init__()
        c7 = _w(c7)
        self.branch1x1 = BasicConv2d(cin, _w(192), kernel_size=1)
        self.branch7x7_1 = BasicConv2d(cin, c7, kernel_size=1)
        self.branch7x7_2 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c7, _w(192), kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(cin, c7, kernel_size=1)
        self.branch7x7dbl_2 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c7, _w(192), kernel_size=(1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(cin, _w(192), kernel_size=1)

    def forward(self, x):
        a = self.branch1x1(x)
        b = self.branch7x7_3(self.branch7x7_2(self.branch7x7_1(x)))
        c = self.branch7x7dbl_5(self.branch7x7dbl_4(self.branch7x7dbl_3(self.branch7x7dbl_2(self.branch7x7dbl_1(x)))))
        d = self.branch_pool(F.avg_pool2d(x, kernel_size=3, stride=1, padding=1))
        return torch.cat([a, b, c, d], 1)


class BlockD(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3_1 = BasicConv2d(cin, _w(192), kernel_size=1)
        self.branch3x3_2 = BasicConv2d(_w(192), _w(320), kernel_size=3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(cin, _w(192), kernel_size=1)
        self.branch7x7x3_2 = BasicConv2d(_w(192), _w(192), kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(_w(192), _w(192), kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(_w(192), _w(192), kernel_size=3, stride=2)

    def forward(self, x):
        a = self.branch3x3_2(self.branch3x3_1(x))
        b = self.branch7x7x3_4(self.branch7x7x3_3(self.branch7x7x3_2(self.branch7x7x3_1(x))))
        return torch.cat([a, b, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


class BlockE(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, _w(320), kernel_size=1)
        self.branch3x3_1 = BasicConv2d(cin, _w(384), kernel_size=1)
        self.branch3x3_2a = BasicConv2d(_w(384), _w(384), kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(_w(384), _w(384), kernel_size=(3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(cin, _w(448), kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(_w(448), _w(384), kernel_size=3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(_w(384), _w(384), kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(_w(384), _w(384), kernel_size=(3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(cin, _w(192), kernel_size=1)

    def forward(self, x):
        a = self.branch1x1(x)
        b = self.branch3x3_1(x)
        b = torch.cat([self.branch3x3_2a(b), self.branch3x3_2b(b)], 1)
        c = self.branch3x3dbl_2(self.branch3x3dbl_1(x))
        c = torch.cat([self.branch3x3dbl_3a(c), self.branch3x3dbl_3b(c)], 1)
        d = self.branch_pool(F.avg_pool2d(x, kernel_size=3, stride=1, padding=1))
        return torch.cat([a, b, c, d], 1)


class NarrowInception(nn.Module):
    def __init__(self):
        super().__init__()
        self.Conv2d_1a_3x3 = BasicConv2d(3, _w(32), kernel_size=3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(_w(32), _w(32), kernel_size=3)
        self.Conv2d_2b_3x3 = BasicConv2d(_w(32), _w(64), kernel_size=3, padding=1)
        self.Conv2d_3b_1x1 = BasicConv2d(_w(64), _w(80), kernel_size=1)
        self.Conv2d_4a_3x3 = BasicConv2d(_w(80), _w(192), kernel_size=3)
        self.Mixed_5b = BlockA(_w(192), 32)
        self.Mixed_5c = BlockA(_w(256), 64)
        self.Mixed_5d = BlockA(_w(288), 64)
        self.Mixed_6a = BlockB(_w(288))
        self.Mixed_6b = BlockC(_w(768), 128)
        self.Mixed_6c = BlockC(_w(768), 160)
        self.Mixed_6d = BlockC(_w(768), 160)
        self.Mixed_6e = BlockC(_w(768), 192)
        self.Mixed_7a = BlockD(_w(768))
        self.Mixed_7b = BlockE(_w(1280))
        self.Mixed_7c = BlockE(_w(2048))
        self.fc = nn.Linear(_w(2048), 10)  # (the reference replaces it by the identity; the loader must ignore it)


def narrow_inception():
    """The seeded module in float32 (convolution weights on the float16 grid), eval mode."""
    state = torch.get_rng_state()
    torch.manual_seed(SEED)
    net = NarrowInception()
    for m in net.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode="fan_in", nonlinearity="relu")
            m.weight.data = m.weight.data.half().float()
        elif isinstance(m, nn.BatchNorm2d):
            nn.init.uniform_(m.weight, 0.7, 1.3)
            nn.init.uniform_(m.bias, -0.2, 0.3)
            m.running_mean.normal_(0.0, 0.2)
            m.running_var.uniform_(0.6, 1.4)
    torch.set_rng_state(state)
    return net.eval()


def stub_inception_v3(weights=None, transform_input=False, **_kw):
    assert transform_input is False
    net = narrow_inception().to(MODE["dtype"])
    return net.to(memory_format=torch.channels_last) if MODE["channels_last"] else net


# ---- torchvision.transforms.functional, restated ----------------------------------------------------------------------------------
class InterpolationMode(enum.Enum):
    BILINEAR = "bilinear"
    BICUBIC = "bicubic"


def tf_resize(img, size, interpolation=InterpolationMode.BILINEAR, antialias=True):
    assert isinstance(size, int) and interpolation is InterpolationMode.BICUBIC and antialias
    h, w = img.shape[-2:]
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    new_w, new_h = (new_short, new_long) if w <= h else (new_long, new_short)
    if (new_h, new_w) == (h, w):
        return img
    if MODE["resize"] == "plain":  # the WRONG resize of the generator's own negative check: a = -0.75, no antialias path
        return F.interpolate(img, size=(new_h, new_w), mode="bicubic", align_corners=False)
    return F.interpolate(img, size=(new_h, new_w), mode="bicubic", align_corners=False, antialias=True)  # (no clamp for float images)


def tf_center_crop(img, output_size):
    ch, cw = output_size
    h, w = img.shape[-2:]
    assert h >= ch and w >= cw
    top, left = int(round((h - ch) / 2.0)), int(round((w - cw) / 2.0))
    return img[..., top: top + ch, left: left + cw]


def tf_normalize(tensor, mean, std):
    if tensor.size(-3) != len(mean):
        raise ValueError("normalize: channel count does not match the mean")
    mean = torch.as_tensor(mean, dtype=tensor.dtype).view(-1, 1, 1)
    std = torch.as_tensor(std, dtype=tensor.dtype).view(-1, 1, 1)
    out = (tensor - mean) / std
    return out.contiguous(memory_format=torch.channels_last) if MODE["channels_last"] else out


def _reference_metrics():
    tv = types.ModuleType("torchvision")
    tvm = types.ModuleType("torchvision.models")
    tvt = types.ModuleType("torchvision.transforms")
    tvf = types.ModuleType("torchvision.transforms.functional")
    tvm.inception_v3 = stub_inception_v3
    tvm.Inception_V3_Weights = types.SimpleNamespace(DEFAULT=None)
    tvm.vgg16, tvm.VGG16_Weights = None, None
    tvf.resize, tvf.center_crop, tvf.normalize, tvf.InterpolationMode = tf_resize, tf_center_crop, tf_normalize, InterpolationMode
    tvt.functional, tv.models, tv.transforms = tvf, tvm, tvt
    sys.modules.update({"torchvision": tv, "torchvision.models": tvm, "torchvision.transforms": tvt, "torchvision.transforms.functional": tvf})
    spec = importlib.util.spec_from_file_location("_ref_metrics", os.path.join(REF, "utils", "metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- inputs, all from seeds -----------------------------------------------------------------------------------------------
def stack_input(seed, shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(int(seed)))


def raw_images(seed, shape, smooth=4, gain=1.25):
    """Images with structure: uniform noise on a grid `smooth` times coarser, enlarged bilinearly, plus fine noise; scaled to
    [-gain, gain] so that some pixels leave [-1, 1] (the pipeline's clamp acts)."""
    g = torch.Generator().manual_seed(int(seed))
    n, c, h, w = shape
    coarse = torch.rand((n, c, -(-h // smooth), -(-w // smooth)), generator=g)
    img = F.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=False) + 0.15 * torch.rand(shape, generator=g)
    return ((img / 1.15) * 2 - 1) * gain


def fid_sets(seed=SEED + 100, n=FID_N, side=FID_SIDE):
    """(real, fake): two sets with different statistics (the fake one is smoother, darker and less saturated)."""
    real = raw_images(seed, (n, 3, side, side), smooth=4, gain=1.25)
    fake = raw_images(seed + 1, (n, 3, side, side), smooth=8, gain=0.9) - 0.1
    return real, fake


def main():
    M = _reference_metrics()
    out = {}
    net = narrow_inception()
    nparams = 0
    for k, v in net.state_dict().items():
        nparams += v.numel()
        if k.endswith("conv.weight"):
            assert torch.equal(v.half().float(), v)
            out[f"sd.{k}"] = v.half().numpy()
        else:
            out[f"sd.{k}"] = v.numpy().copy()
    print(f"narrow Inception: {nparams} state_dict elements, feature dimension {_w(2048)}")

    def mode(dtype=torch.float32, channels_last=False, resize="antialias"):
        MODE.update(dtype=dtype, channels_last=channels_last, resize=resize)

    with torch.no_grad():
        for i, (tag, shape) in enumerate(STACK_CASES):
            seed = SEED + 10 + i
            x = stack_input(seed, shape)
            out[f"stack.{tag}.seed"], out[f"stack.{tag}.shape"] = np.array(seed), np.array(shape)
            for prec, dtype in (("f32", torch.float32), ("f64", torch.float64)):
                mode(dtype)
                out[f"stack.{tag}.{prec}"] = M.InceptionV3(device="cpu")(x.to(dtype)).numpy()
            err = np.abs(out[f"stack.{tag}.f32"] - out[f"stack.{tag}.f64"]).max()
            print(f"stack {tag}: features max {np.abs(out[f'stack.{tag}.f64']).max():.3f}, mean {out[f'stack.{tag}.f64'].mean():.3f}, "
                  f"zeros {(out[f'stack.{tag}.f64'] == 0).mean():.3f}, fp32 max error {err:.2e}")
        for i, (tag, shape) in enumerate(FEAT_CASES):
            seed = SEED + 20 + i
            x = raw_images(seed, shape)
            assert x.min() < -1 and x.max() > 1
            out[f"feat.{tag}.seed"], out[f"feat.{tag}.shape"] = np.array(seed), np.array(shape)
            for prec, dtype in (("f32", torch.float32), ("f64", torch.float64)):
                mode(dtype)
                out[f"feat.{tag}.{prec}"] = M.extract_inception_features(x.to(dtype), device="cpu", batch_size=128)
            print(f"feat {tag}: fp32 max error {np.abs(out[f'feat.{tag}.f32'] - out[f'feat.{tag}.f64']).max():.2e}")

    real, fake = fid_sets()
    out["fid.seed"], out["fid.n"], out["fid.side"] = np.array(SEED + 100), np.array(FID_N), np.array(FID_SIDE)
    mode()
    ref = M.calculate_fid(real, fake, device="cpu", batch_size=128)
    mode(torch.float64)
    f64 = M.calculate_fid(real.double(), fake.double(), device="cpu", batch_size=128)
    feats = [M.extract_inception_features(t.double(), device="cpu", batch_size=128) for t in (real, fake)]
    assert abs(M.fid_from_features(feats[0], feats[1]) - f64) <= 1e-9 * f64
    feats = [f[:, :48].astype(np.float32) for f in feats]
    from_features = M.fid_from_features(feats[0].astype(np.float64), feats[1].astype(np.float64))
    mode(channels_last=True)
    cl = M.calculate_fid(real, fake, device="cpu", batch_size=128)
    mode(resize="plain")
    no_aa = M.calculate_fid(real, fake, device="cpu", batch_size=128)
    mode()
    no_denorm = M.calculate_fid(real * 2 - 1, fake * 2 - 1, device="cpu", batch_size=128)  # (0.5 (2 x - 1) + 0.5 = x: the step undone)
    yard = max(abs(ref - f64), abs(cl - f64))
    print(f"FID ref {ref:.9f}  f64 {f64:.9f}  channels_last {cl:.9f}  of 48 dimensions {from_features:.9f}")
    print(f"yardstick {yard:.3e} ({yard / f64:.2e} of the FID); no antialias {no_aa:.6f}, no denormalize {no_denorm:.6f}")
    assert yard < 1e-3 * f64, "pick other inputs: the fp32 runs disagree too much"
    bound = 4 * yard
    assert abs(no_aa - ref) > 10 * bound and abs(no_denorm - ref) > 10 * bound, "the wrong pipelines must be told apart"
    out.update({"fid.ref": np.array(ref), "fid.f64": np.array(f64), "fid.f32_cl": np.array(cl), "fid.from_features": np.array(from_features),
                "fid.yardstick": np.array(yard), "fid.no_antialias": np.array(no_aa), "fid.no_denorm": np.array(no_denorm),
                "fid.features": np.stack(feats)})
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} keys={len(out)} bytes={os.path.getsize(OUT)}")


if __name__ == "__main__":
    main()

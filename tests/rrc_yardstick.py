"""Yardsticks of tests/test_rrc_host.py and tests/test_rrc_device.py, restated here and never imported from movae_amd: PIL's 8-bit
bicubic resample (coefficient table in float64, 22-bit fixed point, horizontal pass rounded to bytes before the vertical one),
torchvision's RandomResizedCrop.get_params on Philox draws, and the stream layout of those draws.  tests/golden/generate_rrc.py asserts
this resample against PIL itself on every case of the fixture."""
import math

import numpy as np

import data_yardstick as Y

PRECISION_BITS = 22
SCALE, RATIO, TRIES = (0.7, 1.0), (3.0 / 4.0, 4.0 / 3.0), 10


def bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def ksize(in_size, out_size):
    return int(math.ceil(2.0 * max(in_size / out_size, 1.0))) * 2 + 1


def coeffs(in_size, out_size, kmax=None):
    """-> (k int64 [out][kmax], zero past the last tap; bounds int64 [out][2] = (first tap, taps))."""
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    kmax = ksize(in_size, out_size) if kmax is None else kmax
    kk, bounds = np.zeros((out_size, kmax), np.int64), np.zeros((out_size, 2), np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        ss = 1.0 / filterscale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in k:
            ww += w
        if ww != 0.0:
            k = [w / ww for w in k]
        for x, w in enumerate(k):
            kk[xx, x] = int(-0.5 + w * (1 << PRECISION_BITS)) if w < 0 else int(0.5 + w * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return kk, bounds


def resample_axis1(img, out_size):
    """uint8 [n][in][c] -> uint8 [n][out][c] along axis 1; the pass is skipped where in == out."""
    if img.shape[1] == out_size:
        return img
    kk, b = coeffs(img.shape[1], out_size)
    out = np.empty((img.shape[0], out_size, img.shape[2]), np.uint8)
    im = img.astype(np.int64)
    for xx in range(out_size):
        x0, n = b[xx]
        acc = (im[:, x0:x0 + n, :] * kk[xx, :n, None]).sum(1) + (1 << (PRECISION_BITS - 1))
        assert np.abs(acc).max() < 2 ** 31  # the int32 of the C code does not wrap
        out[:, xx, :] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize(crop_hwc, size):
    """PIL's Image.resize((size, size), BICUBIC) of a uint8 HWC image: horizontal, rounded to uint8, then vertical."""
    t = resample_axis1(crop_hwc, size)
    return np.ascontiguousarray(resample_axis1(t.transpose(1, 0, 2), size).transpose(1, 0, 2))


def words(index, stream, seed, epoch):
    """The four Philox words of (index, stream): counter (index, stream, epoch lo, epoch hi), key (seed lo, seed hi)."""
    ctr = np.array([[index & 0xFFFFFFFF, stream, epoch & 0xFFFFFFFF, epoch >> 32]], dtype=np.uint64)
    return [int(v) for v in Y.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))[0]]


def box(index, h, w, seed, epoch):
    """(top, left, bh, bw) of image `index` of h x w: RandomResizedCrop.get_params with try t drawing stream t + 1."""
    for t in range(TRIES):
        w0, w1, w2, w3 = words(index, t + 1, seed, epoch)
        u0, u1 = (w0 + 0.5) / 2.0 ** 32, (w1 + 0.5) / 2.0 ** 32
        area = h * w * (SCALE[0] + (SCALE[1] - SCALE[0]) * u0)
        ar = math.exp(math.log(RATIO[0]) + u1 * (math.log(RATIO[1]) - math.log(RATIO[0])))
        bw, bh = int(round(math.sqrt(area * ar))), int(round(math.sqrt(area / ar)))
        if 0 < bw <= w and 0 < bh <= h:
            return (w2 * (h - bh + 1)) >> 32, (w3 * (w - bw + 1)) >> 32, bh, bw
    in_ratio = w / h
    if in_ratio < RATIO[0]:
        bw, bh = w, int(round(w / RATIO[0]))
    elif in_ratio > RATIO[1]:
        bh, bw = h, int(round(h * RATIO[1]))
    else:
        bw, bh = w, h
    return (h - bh) // 2, (w - bw) // 2, bh, bw


def boxes(dims, seed, epoch):
    return np.array([box(i, int(h), int(w), seed, epoch) for i, (h, w) in enumerate(dims)], dtype=np.int32)


def pack(images, lead=0):
    """uint8 HWC images -> (flat blob, int64 index [N][3] of (byte offset, h, w)), back to back behind `lead` bytes of 0xAA."""
    index, off = [], lead
    for im in images:
        index.append((off, im.shape[0], im.shape[1]))
        off += im.size
    return np.concatenate([np.full(lead, 0xAA, np.uint8)] + [im.reshape(-1) for im in images]), np.array(index, dtype=np.int64)


def load_cases(fx):
    """The cases of tests/golden/rrc_tiny.npz -> list of dicts (src uint8 HWC, box, s, out = PIL's uint8 [s][s][c])."""
    n = int(fx["n_cases"])
    return [dict(src=fx[f"src_{k}"], box=tuple(int(v) for v in fx[f"box_{k}"]), s=int(fx[f"out_{k}"].shape[0]), out=fx[f"out_{k}"])
            for k in range(n)]


def item(image_hwc, box4, size, normalize, flip):
    """The reference's per-item pipeline: crop -> resize -> [flip] -> ToTensor -> [Normalize]  -> CHW float32."""
    top, left, bh, bw = (int(v) for v in box4)
    return Y.transform(resize(image_hwc[top:top + bh, left:left + bw], size), normalize, flip)

"""Image grids as bytes (csrc/visual.hip, movae_amd/visual.py): the geometry on the CPU, the kernel against a numpy restatement of
include/movae.h's rule, byte for byte.  The restatement is fp32 with one rounding per operation and a true division."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F = np.float32
RAW, RANGE, MINMAX = 0, 1, 2


def quantise(v):
    q = np.asarray(v, dtype=F) * F(255) + F(0.5)
    q = np.where(np.isnan(q), F(0), q)
    return np.minimum(np.maximum(q, F(0)), F(255)).astype(np.uint8)


def normalise(x, lo, hi, divide=True):
    lo, hi = F(lo), F(hi)
    den = np.maximum(hi - lo, F(1e-5))
    num = np.minimum(np.maximum(x, lo), hi) - lo
    return (num / den if divide else num * (F(1) / den)).astype(F)


def ref_grid(x, nrow=8, padding=2, mode=RAW, lo=0.0, hi=0.0, pad_value=0.0, divide=True):
    x = np.asarray(x, dtype=F)
    n, c, h, w = x.shape
    if mode == MINMAX:
        lo, hi = x.min(), x.max()
    v = x if mode == RAW else normalise(x, lo, hi, divide)
    b = quantise(v)
    if c == 1:
        b = np.repeat(b, 3, axis=1)
    if n == 1:
        return np.ascontiguousarray(b[0].transpose(1, 2, 0))
    xmaps = min(nrow, n)
    ymaps = -(-n // xmaps)
    H, W = ymaps * (h + padding) + padding, xmaps * (w + padding) + padding
    out = np.full((H, W, 3), quantise(F(pad_value)), dtype=np.uint8)
    for k in range(n):
        y0, x0 = (k // xmaps) * (h + padding) + padding, (k % xmaps) * (w + padding) + padding
        out[y0:y0 + h, x0:x0 + w] = b[k].transpose(1, 2, 0)
    return out


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_grid_shape_by_hand():
    import movae_amd  # noqa: F401
    from movae_amd.visual import grid_shape

    assert grid_shape(5, 3, 5, 3, 2) == (2 * 5 + 2, 3 * 7 + 2) == (12, 23)   # a partly empty last row
    assert grid_shape(3, 4, 6, 8, 2) == (4 + 4, 3 * 8 + 2) == (8, 26)         # n < nrow: three columns, not eight
    assert grid_shape(16, 32, 32, 4, 2) == (4 * 34 + 2, 4 * 34 + 2)
    assert grid_shape(1, 7, 9, 8, 2) == (7, 9)                                # a single image has no border
    assert grid_shape(4, 2, 3, 1, 0) == (8, 3)                                # the per-image dump
    assert grid_shape(8, 32, 32, 4, 2) == (70, 138)                           # the reconstruction figure of four pairs
    for bad in ((0, 1, 1, 1, 0), (1, 0, 1, 1, 0), (1, 1, 1, 0, 0), (1, 1, 1, 1, -1)):
        with pytest.raises(ValueError):
            grid_shape(*bad)


def test_restatement_against_two_grids_written_by_hand():
    # 2 x 1 x 1 x 1, padding 1, grey padding: 0.5 * 255 + 0.5 = 128; 0 -> 0; 1 -> 255.5 -> 255
    g = ref_grid(np.array([0.0, 1.0], dtype=F).reshape(2, 1, 1, 1), nrow=8, padding=1, pad_value=0.5)
    want = np.array([[128, 128, 128, 128, 128], [128, 0, 128, 255, 128], [128, 128, 128, 128, 128]], dtype=np.uint8)
    assert g.shape == (3, 5, 3) and all((g[..., ch] == want).all() for ch in range(3))
    # 3 x 3 x 1 x 2, nrow 2, padding 1, value range (0, 2): x 0 -> 0, 1 -> 128, 2 -> 255, 3 -> 255 (clamped), -1 -> 0 (clamped)
    x = np.array([[[0, 1]], [[2, 3]], [[-1, 1]],
                  [[2, 2]], [[0, 0]], [[1, 1]],
                  [[1, 0]], [[1, 0]], [[1, 2]]], dtype=F).reshape(3, 3, 1, 2)
    g = ref_grid(x, nrow=2, padding=1, mode=RANGE, lo=0.0, hi=2.0)
    o = (0, 0, 0)
    want = np.array([[o] * 7,
                     [o, (0, 255, 0), (128, 255, 128), o, (255, 0, 128), (255, 0, 128), o],
                     [o] * 7,
                     [o, (128, 128, 128), (0, 0, 255), o, o, o, o],
                     [o] * 7], dtype=np.uint8)
    assert g.shape == (5, 7, 3) and (g == want).all()


def test_division_and_reciprocal_give_different_bytes():
    """Why the kernel test on this set means a real division: numpy's two forms disagree on it."""
    u = np.unique(np.linspace(0, 3, 200001).astype(F))
    a, b = quantise(normalise(u, 0, 3, True)), quantise(normalise(u, 0, 3, False))
    print("bytes that differ:", int((a != b).sum()))
    assert (a != b).any()


def test_new_flags_parse():
    import movae_amd  # noqa: F401
    from movae_amd import train

    assert train.parse_args([]).vis == "off"
    a = train.parse_args(["--vis", "on", "--num_vis_samples", "6", "--save_freq", "3"])
    assert (a.vis, a.num_vis_samples, a.save_freq) == ("on", 6, 3)
    with pytest.raises(SystemExit):
        train.parse_args(["--vis", "maybe"])


def test_image_grid_refuses_a_cpu_tensor():
    import movae_amd  # noqa: F401
    from movae_amd import visual

    with pytest.raises(RuntimeError):
        visual.image_grid(torch.zeros(2, 3, 4, 4))


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------
def _modes():
    return [("raw", dict(normalize=False), dict(mode=RAW)),
            ("range", dict(normalize=True, value_range=(-1, 1)), dict(mode=RANGE, lo=-1.0, hi=1.0)),
            ("minmax", dict(normalize=True), dict(mode=MINMAX))]


def _check(x_dev, x_np, kw, ref_kw, **geom):
    from movae_amd import visual

    got = visual.image_grid(x_dev, **geom, **kw)
    want = ref_grid(x_np, **geom, **ref_kw)
    n, _, h, w = x_np.shape
    assert got.dtype == torch.uint8
    assert tuple(got.shape) == want.shape == (*visual.grid_shape(n, h, w, geom.get("nrow", 8), geom.get("padding", 2)), 3)
    bad = int((got.cpu().numpy() != want).sum())
    assert bad == 0, f"{bad} of {want.size} bytes differ"


def _base(seed=0, shape=(5, 3, 3, 5)):
    return (np.random.default_rng(seed).random(shape, dtype=F) * F(3) - F(1.5)).astype(F)  # [-1.5, 1.5): both clamps are met


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["nchw", "channels_last", "sliced"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_base_case_every_layout_and_mode(gpu_device, layout, mode):
    """n 5, c 3, h 3, w 5, nrow 3, padding 2: a row of 69 bytes, one empty cell."""
    x = _base()
    t = torch.from_numpy(x).to(gpu_device)
    if layout == "channels_last":
        t = t.contiguous(memory_format=torch.channels_last)
        assert t.stride() != t.contiguous().stride()
    elif layout == "sliced":
        big = torch.full((10, 3, 3, 5), 99.0, device=gpu_device)  # the rows between must not be read (they would move min / max)
        big[::2] = t
        t = big[::2]
        assert not t.is_contiguous()
    _, kw, ref_kw = _modes()[mode]
    _check(t, x, kw, ref_kw, nrow=3, padding=2)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_one_channel_single_image_and_the_per_image_dump(gpu_device, mode):
    from movae_amd import visual

    _, kw, ref_kw = _modes()[mode]
    x1 = _base(1, (5, 1, 3, 5))
    _check(torch.from_numpy(x1).to(gpu_device), x1, kw, ref_kw, nrow=3, padding=2)       # c == 1: all three channels
    xs = _base(2, (1, 3, 3, 5))
    _check(torch.from_numpy(xs).to(gpu_device), xs, kw, ref_kw, nrow=3, padding=2)       # n == 1: the image, no border
    x = _base(3, (4, 3, 5, 7))
    t = torch.from_numpy(x).to(gpu_device)
    _check(t, x, kw, ref_kw, nrow=1, padding=0)
    dump = visual.to_uint8_batch(t, **kw)
    assert tuple(dump.shape) == (4, 5, 7, 3)
    assert torch.equal(dump.reshape(20, 7, 3), visual.image_grid(t, nrow=1, padding=0, **kw))
    per_image = quantise(x if mode == 0 else normalise(x, *((-1, 1) if mode == 1 else (x.min(), x.max())))).transpose(0, 2, 3, 1)
    assert (dump.cpu().numpy() == per_image).all()


@pytest.mark.gpu
@pytest.mark.parametrize("pad_value", [0.0, 1.0, 0.5])
def test_pad_value_is_quantised_not_normalised(gpu_device, pad_value):
    x = _base(4)
    t = torch.from_numpy(x).to(gpu_device)
    for _, kw, ref_kw in _modes():
        _check(t, x, dict(kw, pad_value=pad_value), dict(ref_kw, pad_value=pad_value), nrow=3, padding=2)
        _check(t, x, dict(kw, pad_value=pad_value), dict(ref_kw, pad_value=pad_value), nrow=2, padding=1)


@pytest.mark.gpu
def test_minmax_range_is_shared_by_the_batch_and_survives_a_constant(gpu_device):
    _, kw, ref_kw = _modes()[2]
    x = (np.random.default_rng(5).random((5, 3, 3, 5), dtype=F)).astype(F)
    x[0, 1, 2, 3], x[3, 2, 0, 4] = F(-2), F(4)  # the minimum in one image, the maximum in another
    _check(torch.from_numpy(x).to(gpu_device), x, kw, ref_kw, nrow=3, padding=2)
    const = np.full((5, 3, 3, 5), 0.7, dtype=F)  # the divisor is 1e-5 and every byte 0
    from movae_amd import visual

    got = visual.image_grid(torch.from_numpy(const).to(gpu_device), nrow=3, padding=2, normalize=True)
    assert int(got.max()) == 0
    _check(torch.from_numpy(const).to(gpu_device), const, kw, ref_kw, nrow=3, padding=2)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["first_last", "middle_first", "last_middle"])
def test_minmax_over_many_partial_blocks(gpu_device, where):
    """2^18 elements: the range is decided by more than one block's partial."""
    x = (np.random.default_rng(6).random((4, 1, 256, 256), dtype=F) * F(0.6) + F(0.2)).astype(F)
    flat = x.reshape(-1)
    assert flat.size == 1 << 18
    lo_at, hi_at = {"first_last": (0, flat.size - 1), "middle_first": (flat.size // 2 + 77, 0),
                    "last_middle": (flat.size - 1, flat.size // 2 - 1234)}[where]
    flat[lo_at], flat[hi_at] = F(-3), F(5)
    _, kw, ref_kw = _modes()[2]
    _check(torch.from_numpy(x).to(gpu_device), x, kw, ref_kw, nrow=2, padding=2)


@pytest.mark.gpu
def test_the_normalisation_divides(gpu_device):
    u = np.unique(np.linspace(0, 3, 200001).astype(F))
    x = u.reshape(1, 1, 1, -1)
    _check(torch.from_numpy(x).to(gpu_device), x, dict(normalize=True, value_range=(0, 3)), dict(mode=RANGE, lo=0.0, hi=3.0))
    from movae_amd import visual

    got = visual.image_grid(torch.from_numpy(x).to(gpu_device), normalize=True, value_range=(0, 3)).cpu().numpy()[0, :, 0]
    assert (got != quantise(normalise(u, 0, 3, divide=False))).any()


@pytest.mark.gpu
def test_nan_pixel_writes_zero(gpu_device):
    from movae_amd import visual

    x = torch.full((2, 3, 2, 2), 0.5, device=gpu_device)
    x[1, 0, 1, 1] = float("nan")
    for kw in (dict(), dict(normalize=True, value_range=(0, 1))):
        g = visual.image_grid(x, nrow=2, padding=0, **kw)
        assert int(g[1, 3, 0]) == 0 and int(g[1, 3, 1]) == 128 and int(g[0, 0, 0]) == 128


@pytest.mark.gpu
def test_refusals(gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import _lib as L

    lib = L.load()
    x = torch.zeros(2, 3, 4, 4, device=gpu_device)
    out = torch.full((64, 64, 3), 7, dtype=torch.uint8, device=gpu_device)
    ws = L.workspace(gpu_device)
    need = lib.movae_image_grid_ws_bytes(2, 3, 4, 4)
    assert 0 < need <= ws.numel() and lib.movae_image_grid_ws_bytes(0, 3, 4, 4) == 0
    st = L.stream_ptr(gpu_device)

    def call(xp=x.data_ptr(), n=2, c=3, h=4, w=4, nrow=2, padding=2, mode=0, lo=0.0, hi=1.0, outp=out.data_ptr(), wsp=ws.data_ptr(),
             wsb=ws.numel()):
        return lib.movae_image_grid_u8(xp, *x.stride(), n, c, h, w, nrow, padding, 0.0, mode, lo, hi, outp, wsp, wsb, st)

    EINVAL = -1
    bad = [dict(xp=None), dict(outp=None), dict(wsp=None, mode=2), dict(n=0), dict(h=0), dict(w=-1), dict(nrow=0), dict(padding=-1),
           dict(c=2), dict(c=4), dict(mode=3), dict(mode=-1), dict(mode=1, lo=1.0, hi=0.5), dict(mode=2, wsb=need - 1)]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert lib.movae_last_error()
    torch.cuda.synchronize()
    assert int(out.min()) == 7  # nothing was launched
    assert call() == 0 and call(mode=1) == 0 and call(mode=2) == 0 and call(mode=0, wsp=None, wsb=0) == 0
    torch.cuda.synchronize()
    flat = out.reshape(-1)  # the picture is 8 x 14 x 3 bytes from the start of the buffer
    assert int(flat[:8 * 14 * 3].max()) == 0 and int(flat[8 * 14 * 3:].min()) == 7

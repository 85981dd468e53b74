"""LPIPS of the final evaluation (movae_amd/metrics.py lpips / lpips_into, csrc/lpips.hip, perceptual.LpipsFeatures): on the CPU the
registration rules of the conv4 block, the refusals and the C-ABI names; on the GPU the distance kernel against a float64 restatement on
the same fp32 inputs, metrics.lpips against values recorded from the reference's own lpips() around a narrow VGG16
(tests/golden/generate_lpips.py), the accumulator's chunks and one training run whose `final:` line carries the value.

Bounds.  Distance kernel: absolute 1e-5 on per-image values in [0, 2] -- normalised components are <= 1 with a few ulp of error each, so
the error of sum (a - b)^2 over d channels stays below about 60 eps sqrt(d) <= 5e-6.  Fixture: the truth is the reference in fp64; the
deviation may be at most 4 x the reference's own recorded fp32-vs-fp64 deviation for the case, or 1e-5 absolute, whichever is larger
(ReLU and max are continuous, so no kink exclusion is needed)."""
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

CONVS7 = (0, 2, 5, 7, 10, 12, 14)
CONVS10 = CONVS7 + (17, 19, 21)
KEYS7 = [f"features.{n}.{leaf}" for n in CONVS7 for leaf in ("weight", "bias")]
KEYS10 = [f"features.{n}.{leaf}" for n in CONVS10 for leaf in ("weight", "bias")]
KERNEL_TOL = 1e-5


def T(a):
    return torch.from_numpy(np.asarray(a))


def weights10():
    fx = load_golden("lpips_tiny")
    return {k: T(fx["vgg." + k]) for k in KEYS10}


def weights7():
    w = weights10()
    return {k: w[k] for k in KEYS7}


@pytest.fixture
def registry(monkeypatch):
    """The module's registry, empty at the start and emptied at the end, and no environment fallback."""
    import movae_amd  # noqa: F401
    from movae_amd import perceptual

    monkeypatch.delenv(perceptual.ENV_VAR, raising=False)
    perceptual.use_vgg16_weights(None)
    yield perceptual
    perceptual.use_vgg16_weights(None)


def fixture_pair(fx, name):
    tag, variant = name.rsplit(".", 1)
    if variant == "same":
        real = T(fx[f"{tag}.a.real"])
        return real, real.clone()
    return T(fx[f"{name}.real"]), T(fx[f"{name}.recon"])


# ---- CPU: registration, refusals, C ABI ---------------------------------------------------------------------------------------------
def test_seven_layer_source_registers_without_the_metric(registry):
    registry.use_vgg16_weights(weights7())
    assert list(registry.registered_vgg16_weights().keys()) == KEYS7
    assert registry.registered_vgg16_lpips_weights() is None
    # a source with only part of the conv4 block is a seven-layer source too
    part = dict(weights7())
    part["features.17.weight"], part["features.17.bias"] = weights10()["features.17.weight"], weights10()["features.17.bias"]
    registry.use_vgg16_weights(part)
    assert list(registry.registered_vgg16_weights().keys()) == KEYS7 and registry.registered_vgg16_lpips_weights() is None


def test_ten_layer_source_serves_both(registry):
    w = weights10()
    registry.use_vgg16_weights(w)
    base, ext = registry.registered_vgg16_weights(), registry.registered_vgg16_lpips_weights()
    assert list(base.keys()) == KEYS7 and list(ext.keys()) == KEYS10
    assert all(torch.equal(ext[k], w[k]) and ext[k].dtype == torch.float32 for k in KEYS10)
    assert registry.registered_vgg16_lpips_weights() is ext  # the same object until the registration changes
    registry.use_vgg16_weights(w)
    assert registry.registered_vgg16_lpips_weights() is not ext
    registry.use_vgg16_weights(None)
    assert registry.registered_vgg16_weights() is None and registry.registered_vgg16_lpips_weights() is None


def test_bad_conv4_shapes_name_the_key_and_register_nothing(registry):
    w = weights10()
    bad = dict(w)
    bad["features.19.weight"] = torch.zeros(64, 7, 3, 3)
    with pytest.raises(ValueError, match=r"features\.19\.weight"):
        registry.use_vgg16_weights(bad)
    assert registry.registered_vgg16_weights() is None and registry.registered_vgg16_lpips_weights() is None
    bad = dict(w)
    bad["features.21.bias"] = torch.zeros(63)
    with pytest.raises(ValueError, match=r"features\.21\.bias"):
        registry.use_vgg16_weights(bad)
    # layer 14 feeds a pool in the extended set: Cout % 4 == 0 there, while the seven-layer set alone accepts the same width
    odd = dict(w)
    odd["features.14.weight"], odd["features.14.bias"] = torch.zeros(30, 32, 3, 3), torch.zeros(30)
    odd["features.17.weight"] = torch.zeros(64, 30, 3, 3)
    with pytest.raises(ValueError, match=r"features\.14\.weight"):
        registry.use_vgg16_weights(odd)
    assert registry.registered_vgg16_weights() is None
    registry.use_vgg16_weights({k: odd[k] for k in KEYS7})
    assert registry.registered_vgg16_weights()["features.14.bias"].shape == (30,) and registry.registered_vgg16_lpips_weights() is None


def test_key_prefixes_and_the_environment_fallback(registry, tmp_path, monkeypatch):
    w = weights10()
    forms = [w, {k[len("features."):]: v for k, v in w.items()}, {"perceptual_loss." + k: v for k, v in w.items()}]
    for src in forms:
        got = registry.load_vgg16_lpips_weights(src)
        assert list(got.keys()) == KEYS10 and all(torch.equal(got[k], w[k]) for k in KEYS10)
        assert list(registry.load_vgg16_weights(src).keys()) == KEYS7
    path = tmp_path / "vgg.pt"
    torch.save(w, path)
    monkeypatch.setenv(registry.ENV_VAR, str(path))
    ext = registry.registered_vgg16_lpips_weights()
    assert list(ext.keys()) == KEYS10 and registry.registered_vgg16_lpips_weights() is ext
    assert list(registry.registered_vgg16_weights().keys()) == KEYS7
    registry.use_vgg16_weights(weights7())  # a registration wins over the environment, for the metric too
    assert registry.registered_vgg16_lpips_weights() is None


def test_feature_module_layout(registry):
    f = registry.LpipsFeatures(weights10())
    assert list(f.state_dict().keys()) == [k[len("features."):] for k in KEYS10]
    assert all(p.requires_grad is False for p in f.parameters()) and not f.training
    assert f.train() is f and not f.training
    assert isinstance(getattr(f, "17"), registry._FrozenConv) and issubclass(registry.LpipsFeatures, registry._Features)
    assert registry.LpipsFeatures.pool_after == (2, 7, 14)


def test_refusals_without_a_device(registry):
    from movae_amd import metrics

    x = torch.rand(2, 3, 32, 32)
    with pytest.raises(ValueError, match="Network alex not supported. Currently only 'vgg' is supported."):
        metrics.lpips(x, x, net="alex")
    assert math.isnan(metrics.lpips(torch.zeros(0, 3, 32, 32), x))
    assert math.isnan(metrics.lpips(x, torch.zeros(0, 3, 32, 32)))
    with pytest.raises(RuntimeError, match=r"perceptual\.use_vgg16_weights"):
        metrics.lpips(x, x)
    registry.use_vgg16_weights(weights7())
    with pytest.raises(RuntimeError, match=r"perceptual\.use_vgg16_weights"):
        metrics.lpips(x, x)


def test_c_abi_names():
    import movae_amd  # noqa: F401
    from movae_amd import _lib, build

    hdr = open(os.path.join(ROOT, "include", "movae.h")).read()
    for name in ("movae_lpips_ws_bytes", "movae_lpips_layer", "movae_lpips_finalize"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES
    assert "lpips.hip" in build.SOURCES
    lib = movae_amd.load_library()
    assert lib.movae_lpips_ws_bytes(2, 4, 4, 64) >= 2 * 8 and lib.movae_lpips_ws_bytes(2, 4, 4, 64) % 256 == 0
    assert lib.movae_lpips_ws_bytes(2, 4, 4, 6) == 0  # c % 4 != 0: no such layer


# ---- GPU: the distance kernel -------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1, 4), (3, 5, 7, 8), (2, 4, 4, 20), (2, 9, 3, 64), (1, 6, 5, 128), (2, 3, 3, 256), (1, 2, 3, 512), (5, 2, 2, 64)]


def feature_pair(shape, seed):
    """Two fp32 NHWC feature maps like a ReLU's output (about half zeros), with -- where the shape has the pixels -- one pixel zero in
    both, one zero in the first only, one zero in the second only and one of size 1e18 in the first."""
    g = torch.Generator().manual_seed(seed)
    f1 = torch.randn(shape, generator=g).clamp_min(0) * 3
    f2 = (f1 + 0.3 * torch.randn(shape, generator=g)).clamp_min(0)
    n, h, w, c = shape
    v1, v2 = f1.view(-1, c), f2.view(-1, c)
    if v1.size(0) >= 4:
        last = v1.size(0) - 1
        v1[0], v2[0] = 0, 0
        v1[1] = 0
        v2[last] = 0
        v1[last - 1] = 1e18 * (0.5 + torch.rand(c, generator=g))
    return f1, f2


def distance_f64(f1, f2):
    """The reference's expression per image (F.normalize's rule with its eps) in float64."""
    a, b = f1.double(), f2.double()
    a = a / a.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    b = b / b.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return ((a - b) ** 2).sum(-1).mean(dim=(1, 2))


def run_distance(pairs, device):
    from movae_amd import metrics

    out = torch.full((1 + pairs[0][0].size(0),), float("nan"), dtype=torch.float32, device=device)
    return metrics.feature_distance_into(out, [(a.to(device), b.to(device)) for a, b in pairs]).cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_distance_kernel_against_float64(shape, gpu_device):
    import movae_amd  # noqa: F401

    f1, f2 = feature_pair(shape, seed=sum(shape))
    want = distance_f64(f1, f2)
    assert (want >= 0).all() and (want <= 2).all()
    got = run_distance([(f1, f2)], gpu_device).double()
    dev = float((got[1:] - want).abs().max())
    print(f"{shape}: per-image values {want.tolist()}, worst deviation {dev:.3g}")
    assert dev <= KERNEL_TOL
    assert abs(float(got[0]) - float(want.mean())) <= KERNEL_TOL
    # identical operands: exactly zero, per image and in the mean; two runs: the same bits; swapped operands: the same value
    same = run_distance([(f1, f1.clone())], gpu_device)
    assert torch.equal(same, torch.zeros_like(same))
    again = run_distance([(f1, f2)], gpu_device)
    assert torch.equal(again.double(), got)
    swapped = run_distance([(f2, f1)], gpu_device)
    assert torch.equal(swapped.double(), got)


@pytest.mark.gpu
def test_distance_over_several_layers_and_refusals(gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import _lib as L

    shapes = [(3, 8, 8, 8), (3, 4, 4, 64), (3, 2, 2, 512), (3, 1, 1, 20)]
    pairs = [feature_pair(s, seed=70 + i) for i, s in enumerate(shapes)]
    want = torch.stack([distance_f64(a, b) for a, b in pairs]).mean(0)
    got = run_distance(pairs, gpu_device).double()
    assert float((got[1:] - want).abs().max()) <= KERNEL_TOL and abs(float(got[0]) - float(want.mean())) <= KERNEL_TOL
    a = torch.zeros(1, 2, 2, 6, device=gpu_device)
    part = torch.zeros(64, dtype=torch.float64, device=gpu_device)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        L.call("movae_lpips_layer", a.data_ptr(), a.data_ptr(), 1, 2, 2, 6, 1.0, part.data_ptr(), part.numel() * 8, L.stream_ptr(gpu_device))
    b = torch.zeros(1, 2, 2, 8, device=gpu_device)
    with pytest.raises(RuntimeError, match="partials hold"):
        L.call("movae_lpips_layer", b.data_ptr(), b.data_ptr(), 1, 2, 2, 8, 1.0, part.data_ptr(), 8, L.stream_ptr(gpu_device))


# ---- GPU: metrics.lpips against the reference's recorded values ----------------------------------------------------------------------
FIXTURE_CASES = [f"{tag}.{v}" for tag in ("3x3x32x32", "2x3x40x36", "2x1x32x32") for v in ("a", "b", "same")]


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_lpips_against_the_reference(name, registry, gpu_device):
    from movae_amd import metrics

    fx = load_golden("lpips_tiny")
    assert list(fx["cases"]) == FIXTURE_CASES
    registry.use_vgg16_weights(weights10())
    real, recon = fixture_pair(fx, name)
    truth, yard = float(fx[f"{name}.lpips.f64"]), float(fx[f"{name}.lpips.f32"])
    got = metrics.lpips(real.to(gpu_device), recon.to(gpu_device))
    bound = max(4 * abs(yard - truth), 1e-5)
    print(f"{name}: lpips {got:.9f}, reference fp64 {truth:.9f}, error {abs(got - truth):.3g}, reference-fp32 deviation {abs(yard - truth):.3g}")
    assert isinstance(got, float) and abs(got - truth) <= bound
    if name.endswith(".same"):
        assert got == 0.0 and truth == 0.0
    # `device` moves host operands; the result is the same number
    assert metrics.lpips(real, recon, device=gpu_device) == got


@pytest.mark.gpu
def test_lpips_refusals_on_the_device(registry, gpu_device):
    from movae_amd import metrics

    x = torch.rand(2, 3, 32, 32, device=gpu_device)
    with pytest.raises(RuntimeError, match=r"perceptual\.use_vgg16_weights"):
        metrics.lpips(x, x)
    registry.use_vgg16_weights(weights10())
    for shape in ((2, 3, 7, 32), (2, 3, 32, 6)):
        small = torch.rand(shape, device=gpu_device)
        with pytest.raises(ValueError, match="at least 8 x 8"):
            metrics.lpips(small, small)
    assert metrics.lpips(torch.rand(1, 3, 8, 8, device=gpu_device), torch.rand(1, 3, 8, 8, device=gpu_device)) > 0
    with pytest.raises(ValueError, match="shapes differ"):
        metrics.lpips(x, x[:1])
    # re-registering rebuilds the cached feature extractor: other weights, another value
    y = torch.rand(2, 3, 32, 32, device=gpu_device)
    first = metrics.lpips(x, y)
    registry.use_vgg16_weights({k: (v.flip(0) if k.startswith("features.0.") else v) for k, v in weights10().items()})
    assert metrics.lpips(x, y) != first
    registry.use_vgg16_weights(weights10())
    assert metrics.lpips(x, y) == first


# ---- GPU: the accumulator and the training loop --------------------------------------------------------------------------------------
def _collection(side):
    g = torch.Generator().manual_seed(300 + side)
    real = torch.rand(300, 3, side, side, generator=g)
    recon = torch.tanh(2 * real - 1 + 0.2 * torch.randn(real.shape, generator=g))  # a tanh decoder's output
    return real, recon


def _accumulate(device, real, recon):
    from movae_amd import metrics

    acc = metrics.ReconMetricAccumulator(device, max_samples=10000)
    for i in range(0, real.size(0), 50):
        acc.add(real[i:i + 50].to(device), recon[i:i + 50].to(device))
    assert acc.count == 300
    return acc.result()


@pytest.mark.gpu
def test_accumulator_scores_lpips_per_chunk(registry, gpu_device):
    from movae_amd import metrics

    real, recon = _collection(32)
    plain = _accumulate(gpu_device, real, recon)
    assert math.isnan(plain["lpips"])
    registry.use_vgg16_weights(weights10())
    res = _accumulate(gpu_device, real, recon)
    chunks = [metrics.lpips(real[i:i + 128].to(gpu_device), recon[i:i + 128].to(gpu_device)) for i in (0, 128, 256)]
    print(f"chunks {chunks}, accumulated {res['lpips']}")
    assert abs(res["lpips"] - float(np.mean(chunks))) <= 1e-6 and 0 < res["lpips"] < 2
    assert res["ssim"] == plain["ssim"] and res["psnr"] == plain["psnr"] and math.isnan(res["rfid"])
    # the width gate (the reference's min_size_for_lpips) and a registration without the conv4 block
    small = _accumulate(gpu_device, *_collection(16))
    assert math.isnan(small["lpips"]) and np.isfinite(small["ssim"])
    registry.use_vgg16_weights(weights7())
    seven = _accumulate(gpu_device, real, recon)
    assert math.isnan(seven["lpips"]) and seven["ssim"] == plain["ssim"] and seven["psnr"] == plain["psnr"]


@pytest.mark.gpu
def test_training_run_reports_lpips(registry, gpu_device, tmp_path, capsys):
    from movae_amd import train

    registry.use_vgg16_weights(weights10())
    argv = ["--dataset", "synthetic_cifar10", "--arch", "vae", "--agg", "upgrad", "--batch_size", "50", "--max_items", "500",
            "--latent_dim", "16", "--hidden_dims", "16", "32", "--save_path", str(tmp_path), "--seed", "2", "--device", "cuda:0",
            "--graph", "off", "--epochs", "1", "--eval_freq", "0", "--max_fid_samples", "256"]
    args = train.parse_args(argv)
    train.set_seed(args.seed)
    train.main(args)
    out = capsys.readouterr().out
    final = [ln for ln in out.splitlines() if ln.startswith("final: ")]
    assert len(final) == 1
    rec = train.LAST_FINAL["recon"]
    assert np.isfinite(rec["lpips"]) and 0 < rec["lpips"] < 2
    assert math.isnan(rec["rfid"]) and np.isfinite(rec["ssim"]) and np.isfinite(rec["psnr"])
    m = re.search(r"lpips: ([-+0-9.eE]+)", final[0])
    assert m and float(m.group(1)) == pytest.approx(rec["lpips"], abs=1e-6)
    assert re.search(r"rfid: nan", final[0])

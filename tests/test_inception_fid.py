"""rFID of the final evaluation (movae_amd/inception.py, metrics.fid / inception_features / fid_from_features, csrc/inception.hip).

On the CPU: the weight loader (torchvision's inception_v3 state_dict layout, the BatchNorm fold, the key named on an error), the
registration rules, the Frechet distance against the value recorded from the reference's fid_from_features, and the accumulator's NaN
with nothing registered.  On the GPU: the inference kernels, the input pipeline, the stack and the metric.

The fixture (tests/golden/generate_inception.py, run on the CPU next to the reference) holds a narrow Inception-v3 (1/8 widths, D = 256),
the reference's own features and FID in float32 and float64, and the seeds of every input; the inputs are rebuilt here by the
generator's own functions (imported by path; it touches the reference only inside its main()).

Tolerance of every numeric GPU test: the truth is a float64 restatement (torch on the CPU, or the fixture's float64 run); the error
may be at most 4 x the error of torch's float32 CPU result against that same truth -- the factor covers the different summation order
of a correct fp32 implementation.  Each test prints its ratio before it asserts."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, load_golden


def _generator():
    spec = importlib.util.spec_from_file_location("_gen_inception", os.path.join(GOLDEN, "generate_inception.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _generator()


@pytest.fixture(scope="module")
def fx():
    return load_golden("inception_tiny")


def state_dict(fx):
    return {k[3:]: torch.from_numpy(np.asarray(fx[k])).float() if k.endswith("conv.weight") else torch.from_numpy(np.asarray(fx[k]))
            for k in fx.files if k.startswith("sd.")}


@pytest.fixture
def registry(monkeypatch):
    """The module's registry, empty at the start and emptied at the end, and no environment fallback."""
    import movae_amd  # noqa: F401
    from movae_amd import inception

    monkeypatch.delenv(inception.ENV_VAR, raising=False)
    inception.use_inception_weights(None)
    yield inception
    inception.use_inception_weights(None)


def within(got, truth, cpu32, what, factor=4.0):
    """max |got - truth| <= factor * max |cpu32 - truth|, printed first."""
    got, truth, cpu32 = (torch.as_tensor(t).detach().cpu().double() for t in (got, truth, cpu32))
    assert got.shape == truth.shape == cpu32.shape, (got.shape, truth.shape, cpu32.shape)
    err, base = (got - truth).abs().max().item(), (cpu32 - truth).abs().max().item()
    ratio = err / base if base else (float("inf") if err else 0.0)
    print(f"{what}: error {err:.3e}, torch fp32 CPU {base:.3e}, ratio {ratio:.2f}")
    assert math.isfinite(err) and err <= factor * base, f"{what}: {err:.3e} > {factor} x {base:.3e}"
    return err, base


# ---- CPU: loader, registration, the distance ----------------------------------------------------------------------------------------
def test_loader_accepts_a_torchvision_state_dict(fx, registry):
    sd = state_dict(fx)
    assert any(k.startswith("fc.") for k in sd) and any(k.endswith("num_batches_tracked") for k in sd)
    sd["AuxLogits.conv0.conv.weight"] = torch.zeros(4, 96, 1, 1)
    sd["AuxLogits.fc.bias"] = torch.zeros(10)
    w = registry.load_inception_weights(sd)
    layers = registry.conv_layers()
    assert len(layers) == 94 and len(w) == 3 * 94 and w.feature_dim == 256
    assert [k for k in w][:3] == ["Conv2d_1a_3x3.weight", "Conv2d_1a_3x3.scale", "Conv2d_1a_3x3.shift"]
    assert not any("AuxLogits" in k or k.startswith("fc") for k in w)
    for name, (kh, kw, _, _, _) in layers:
        assert tuple(w[f"{name}.weight"].shape[2:]) == (kh, kw) and w[f"{name}.weight"].dtype == torch.float32
        assert torch.equal(w[f"{name}.weight"], sd[f"{name}.conv.weight"])  # (the weight itself stays unscaled)
    # the reference's wrapper keeps the network under `model.`; a module is accepted as well as a mapping
    assert len(registry.load_inception_weights({"model." + k: v for k, v in sd.items()})) == 3 * 94
    assert len(registry.load_inception_weights(GEN.narrow_inception())) == 3 * 94


def test_loader_names_the_key(fx, registry):
    sd = state_dict(fx)
    for key in ("Mixed_6c.branch7x7dbl_4.conv.weight", "Mixed_7b.branch3x3_2b.bn.running_var", "Conv2d_1a_3x3.bn.weight"):
        part = {k: v for k, v in sd.items() if k != key}
        with pytest.raises(ValueError, match=re.escape(key)):
            registry.load_inception_weights(part)
    bad = dict(sd)
    bad["Mixed_6b.branch7x7_2.conv.weight"] = sd["Mixed_6b.branch7x7_2.conv.weight"].permute(0, 1, 3, 2).contiguous()  # (7, 1) for (1, 7)
    with pytest.raises(ValueError, match=r"Mixed_6b\.branch7x7_2\.conv\.weight has shape"):
        registry.load_inception_weights(bad)
    bad = dict(sd)
    bad["Mixed_5c.branch_pool.bn.bias"] = torch.zeros(9)
    with pytest.raises(ValueError, match=r"Mixed_5c\.branch_pool\.bn\.bias has shape"):
        registry.load_inception_weights(bad)
    bad = dict(sd)  # a width that does not chain: Mixed_5b's pool branch widened, so Mixed_5c sees one channel more than its weights take
    bad["Mixed_5b.branch_pool.conv.weight"] = torch.zeros(5, 24, 1, 1)
    for leaf in ("weight", "bias", "running_mean", "running_var"):
        bad[f"Mixed_5b.branch_pool.bn.{leaf}"] = torch.ones(5)
    with pytest.raises(ValueError, match=r"Mixed_5c\.branch1x1\.conv\.weight has shape"):
        registry.load_inception_weights(bad)


def test_batchnorm_fold_matches_float64(fx, registry):
    sd = state_dict(fx)
    w = registry.load_inception_weights(sd)
    for name, _ in registry.conv_layers():
        g, b, m, v = (sd[f"{name}.bn.{leaf}"].double() for leaf in ("weight", "bias", "running_mean", "running_var"))
        s = g / torch.sqrt(v + 1e-3)
        t = b - m * s
        assert torch.equal(w[f"{name}.scale"], s.float()) and torch.equal(w[f"{name}.shift"], t.float()), name
    assert (w["Mixed_7c.branch_pool.shift"] != 0).any() and (w["Mixed_7c.branch_pool.scale"] != 1).all()


def test_registration_removal_and_environment(fx, registry, monkeypatch, tmp_path):
    assert registry.registered_inception_weights() is None
    sd = state_dict(fx)
    registry.use_inception_weights(sd)
    first = registry.registered_inception_weights()
    assert first is not None and registry.registered_inception_weights() is first
    with pytest.raises(ValueError):
        registry.use_inception_weights({"Conv2d_1a_3x3.conv.weight": torch.zeros(4, 3, 3, 3)})
    assert registry.registered_inception_weights() is first  # (a refused source leaves the registration alone)
    registry.use_inception_weights(None)
    assert registry.registered_inception_weights() is None
    path = tmp_path / "inception.pt"
    torch.save(sd, path)
    monkeypatch.setenv("MOVAE_INCEPTION_WEIGHTS", str(path))
    env = registry.registered_inception_weights()
    assert env is not None and env is registry.registered_inception_weights() and len(env) == 3 * 94
    registry.use_inception_weights(str(path))  # a path registers too, and an explicit registration wins over the environment
    assert registry.registered_inception_weights() is not env
    monkeypatch.delenv("MOVAE_INCEPTION_WEIGHTS")
    registry.use_inception_weights(None)
    assert registry.registered_inception_weights() is None


def test_fid_from_features_matches_the_reference(fx):
    import movae_amd  # noqa: F401
    from movae_amd import metrics

    feats = fx["fid.features"]
    assert feats.shape == (2, 320, 48)  # N > D
    ref = float(fx["fid.from_features"])
    got = metrics.fid_from_features(torch.from_numpy(feats[0]), torch.from_numpy(feats[1]))
    print(f"fid_from_features {got!r}, reference {ref!r}, relative {abs(got - ref) / ref:.2e}")
    assert abs(got - ref) <= 1e-9 * ref
    assert metrics.fid_from_features(feats[0], feats[1]) == got  # (arrays as well as tensors)
    assert abs(metrics.fid_from_features(feats[0], feats[0])) <= 1e-9 * ref
    assert math.isnan(metrics.fid_from_features(feats[0][:0], feats[1]))


def test_accumulator_without_weights_gives_nan(registry, monkeypatch):
    from movae_amd import metrics

    # (the SSIM / PSNR launch needs the GPU; the rFID decision does not)
    monkeypatch.setattr(metrics, "_run", lambda real, recon, window_size=11, max_val=1.0: torch.zeros(3 + 3 * real.size(0)))
    before = dict(metrics._inception_features)
    acc = metrics.ReconMetricAccumulator("cpu", 40, chunk=16)
    for n in (10, 25, 30):
        acc.add(torch.rand(n, 3, 32, 32), torch.rand(n, 3, 32, 32))
    res = acc.result()
    assert acc.count == 40 and math.isnan(res["rfid"]) and res["ssim"] == 0.0
    assert acc._fid is False and acc._feats == ([], []) and metrics._inception_features == before
    with pytest.raises(RuntimeError, match="use_inception_weights"):
        metrics.inception_features_into(torch.empty(2, 256), torch.rand(2, 3, 32, 32))


# ---- GPU: kernels -------------------------------------------------------------------------------------------------------------------
def _conv_case(dev, seed, n, h, w, ci, co, k, stride, pad, ldy=None, offset=0, shift_bias=0.0):
    from movae_amd import ops

    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, ci, h, w), generator=g)
    wt = torch.randn((co, ci) + k, generator=g) / math.sqrt(ci * k[0] * k[1])
    scale = torch.rand(co, generator=g) + 0.5
    shift = torch.randn(co, generator=g) * 0.3 + shift_bias

    def ref(dt):
        y = F.conv2d(x.to(dt), wt.to(dt), stride=stride, padding=pad)
        return torch.relu(y * scale.to(dt).view(1, -1, 1, 1) + shift.to(dt).view(1, -1, 1, 1)).permute(0, 2, 3, 1)

    truth, cpu32 = ref(torch.float64), ref(torch.float32)
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    wd = wt.permute(0, 2, 3, 1).contiguous().to(dev)
    out = None
    if ldy is not None:
        out = torch.full(tuple(truth.shape[:3]) + (ldy,), -7.25, device=dev)
    got = ops.infer_conv2d(xd, wd, scale.to(dev), shift.to(dev), stride, pad, out, offset)
    return got, truth, cpu32


CONV_CASES = {
    # name: (n, h, w, ci, co, (kh, kw), stride, (ph, pw))
    "row7 17x17": (1, 17, 17, 16, 20, (1, 7), 1, (0, 3)),
    "col7 17x17": (1, 17, 17, 16, 20, (7, 1), 1, (3, 0)),
    "row7 5x9 overhang": (2, 5, 9, 16, 20, (1, 7), 1, (0, 3)),
    "col7 5x9 overhang": (2, 5, 9, 16, 20, (7, 1), 1, (3, 0)),
    "row3 3x3": (1, 3, 3, 48, 48, (1, 3), 1, (0, 1)),
    "col3 3x3": (1, 3, 3, 48, 48, (3, 1), 1, (1, 0)),
    "row3 1x1": (2, 1, 1, 48, 48, (1, 3), 1, (0, 1)),
    "col3 1x1": (2, 1, 1, 48, 48, (3, 1), 1, (1, 0)),
    "5x5 p2 6->8 9x9": (1, 9, 9, 6, 8, (5, 5), 1, (2, 2)),
    "3x3 s2 35x35": (1, 35, 35, 12, 24, (3, 3), 2, (0, 0)),
    "3x3 s2 8x7": (2, 8, 7, 12, 56, (3, 3), 2, (0, 0)),
    "stem 3->4 s2 75x75": (1, 75, 75, 3, 4, (3, 3), 2, (0, 0)),    # K = 27
    "stem 3->4 s2 11x10": (2, 11, 10, 3, 4, (3, 3), 2, (0, 0)),
    "n3 7x5 tail": (3, 7, 5, 8, 10, (3, 3), 1, (1, 1)),
    "K42 co10": (1, 6, 6, 6, 10, (1, 7), 1, (0, 3)),               # K = 42, ci % 4 != 0
    "1x1 co24": (2, 9, 8, 10, 24, (1, 1), 1, (0, 0)),
    "1x1 co56 two row tiles": (2, 17, 17, 24, 56, (1, 1), 1, (0, 0)),
    "3x3 co136 wide tile": (1, 9, 9, 8, 136, (3, 3), 1, (1, 1)),    # two column tiles
    "3x3 co70 96-column tile": (2, 9, 9, 8, 70, (3, 3), 1, (1, 1)),
    "1x1 co150 five 32-column tiles": (2, 9, 9, 12, 150, (1, 1), 1, (0, 0)),
    "1x1 co128 128-column tile": (2, 9, 9, 12, 128, (1, 1), 1, (0, 0)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONV_CASES))
def test_infer_conv2d(gpu_device, name):
    n, h, w, ci, co, k, stride, pad = CONV_CASES[name]
    got, truth, cpu32 = _conv_case(gpu_device, 100 + list(CONV_CASES).index(name), n, h, w, ci, co, k, stride, pad)
    assert (truth > 0).any() and (truth == 0).any()
    within(got, truth, cpu32, f"infer_conv2d {name}")


@pytest.mark.gpu
def test_infer_conv2d_writes_only_its_slice(gpu_device):
    got, truth, cpu32 = _conv_case(gpu_device, 7, 2, 9, 7, 16, 12, (3, 3), 1, (1, 1), ldy=40, offset=8)
    assert got.shape[-1] == 40
    within(got[..., 8:20], truth, cpu32, "infer_conv2d slice")
    rest = torch.cat([got[..., :8], got[..., 20:]], -1)
    assert torch.equal(rest, torch.full_like(rest, -7.25))


@pytest.mark.gpu
def test_infer_conv2d_relu_clamps(gpu_device):
    got, truth, cpu32 = _conv_case(gpu_device, 8, 1, 6, 6, 8, 12, (3, 3), 1, (1, 1), shift_bias=-50.0)
    assert (truth == 0).all() and torch.equal(got.cpu(), torch.zeros_like(got.cpu()))


@pytest.mark.gpu
def test_infer_conv2d_refusals(gpu_device):
    from movae_amd import ops

    x = torch.zeros(1, 5, 5, 4, device=gpu_device)
    w = torch.zeros(8, 3, 3, 4, device=gpu_device)
    s = torch.ones(8, device=gpu_device)
    with pytest.raises(ValueError):
        ops.infer_conv2d(x, w, s, s, out=torch.zeros(1, 3, 3, 10, device=gpu_device), offset=4)  # 4 + 8 > 10
    with pytest.raises(ValueError):
        ops.infer_conv2d(x, torch.zeros(8, 3, 3, 5, device=gpu_device), s, s)
    with pytest.raises(RuntimeError, match="padding"):
        ops.infer_conv2d(x, w, s, s, pad=(3, 0))
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.infer_conv2d(x.cpu(), w.cpu(), s.cpu(), s.cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(7, 7), (8, 9)])
@pytest.mark.parametrize("c,ldy,off", [(6, 11, 3), (8, 16, 4)])  # one channel per thread / four (16-byte accesses)
def test_infer_max_pool_into_a_slice(gpu_device, h, w, c, ldy, off):
    from movae_amd import ops

    x = -torch.rand((2, c, h, w), generator=torch.Generator().manual_seed(h * w)) - 0.5  # all negative: a zero-initialised maximum would win
    truth = F.max_pool2d(x, kernel_size=3, stride=2).permute(0, 2, 3, 1)
    out = torch.full(tuple(truth.shape[:3]) + (ldy,), 3.5, device=gpu_device)
    got = ops.infer_pool3x3(x.permute(0, 2, 3, 1).contiguous().to(gpu_device), "max", out, off).cpu()
    assert torch.equal(got[..., off: off + c], truth) and (got[..., :off] == 3.5).all() and (got[..., off + c:] == 3.5).all()


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(1, 1), (3, 3), (5, 4)])
@pytest.mark.parametrize("c", [5, 8])  # one channel per thread / four
def test_infer_avg_pool_divides_by_nine(gpu_device, h, w, c):
    from movae_amd import ops

    x = torch.rand((2, c, h, w), generator=torch.Generator().manual_seed(10 * h + w)) + 0.25
    truth = F.avg_pool2d(x.double(), kernel_size=3, stride=1, padding=1).permute(0, 2, 3, 1)
    cpu32 = F.avg_pool2d(x, kernel_size=3, stride=1, padding=1).permute(0, 2, 3, 1)
    got = ops.infer_pool3x3(x.permute(0, 2, 3, 1).contiguous().to(gpu_device), "avg")
    assert torch.allclose(truth[:, 0, 0], x.double()[:, :, :2, :2].sum((2, 3)) / 9)  # (the corner of the restatement divides by 9)
    within(got, truth, cpu32, f"infer_pool3x3 avg {h}x{w} c{c}")


@pytest.mark.gpu
def test_infer_global_mean(gpu_device):
    from movae_amd import ops

    x = torch.randn((3, 8, 8, 37), generator=torch.Generator().manual_seed(3)) + 0.5
    got = ops.infer_global_mean(x.to(gpu_device))
    within(got, x.double().mean((1, 2)), x.mean((1, 2)), "infer_global_mean")
    one = torch.randn((2, 1, 1, 5), generator=torch.Generator().manual_seed(4))
    assert torch.equal(ops.infer_global_mean(one.to(gpu_device)).cpu(), one.view(2, 5))


# ---- GPU: the input pipeline --------------------------------------------------------------------------------------------------------
def _prep_reference(x):
    """calculate_fid's denormalize + _inception_preprocess in x's dtype, through the generator's restated transforms; -> NHWC."""
    GEN.MODE.update(dtype=x.dtype, channels_last=False, resize="antialias")
    v = (x * 0.5 + 0.5).clamp(0, 1)
    v = GEN.tf_resize(v, 299, interpolation=GEN.InterpolationMode.BICUBIC, antialias=True)
    v = GEN.tf_center_crop(v, [299, 299])
    return GEN.tf_normalize(v, mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225]).permute(0, 2, 3, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,gain", [(32, 32, 1.25), (64, 64, 1.25), (75, 75, 1.0), (256, 256, 1.25), (299, 299, 1.25), (40, 64, 1.25),
                                      (64, 40, 3.0)])
def test_inception_prep(gpu_device, h, w, gain):
    from movae_amd import ops

    x = GEN.raw_images(500 + h + w, (2, 3, h, w), gain=gain)
    assert gain <= 1.0 or (x.min() < -1 and x.max() > 1)  # inputs outside [-1, 1]: the clamp acts
    truth, cpu32 = _prep_reference(x.double()), _prep_reference(x)
    got = ops.inception_prep(x.to(gpu_device))
    assert tuple(got.shape) == (2, 299, 299, 3)
    within(got, truth, cpu32, f"inception_prep {h}x{w}")


@pytest.mark.gpu
def test_inception_prep_refuses_a_side_above_299(gpu_device):
    from movae_amd import ops

    for shape in ((1, 3, 300, 64), (1, 3, 64, 300)):
        with pytest.raises(NotImplementedError, match="299"):
            ops.inception_prep(torch.zeros(shape, device=gpu_device))
    with pytest.raises(ValueError):
        ops.inception_prep(torch.zeros((1, 1, 32, 32), device=gpu_device))


# ---- GPU: the stack and the metric --------------------------------------------------------------------------------------------------
@pytest.fixture
def narrow(fx, registry):
    registry.use_inception_weights(state_dict(fx))
    return registry


@pytest.mark.gpu
@pytest.mark.parametrize("tag", [t for t, _ in GEN.STACK_CASES])
def test_stack_matches_the_reference_features(fx, narrow, gpu_device, tag):
    from movae_amd import metrics

    x = GEN.stack_input(int(fx[f"stack.{tag}.seed"]), tuple(int(v) for v in fx[f"stack.{tag}.shape"]))
    net = metrics._inception_on(gpu_device, narrow.registered_inception_weights())
    got = net(x.permute(0, 2, 3, 1).contiguous().to(gpu_device))
    assert tuple(got.shape) == (x.size(0), 256)
    within(got, fx[f"stack.{tag}.f64"], fx[f"stack.{tag}.f32"], f"stack {tag}")


@pytest.mark.gpu
@pytest.mark.parametrize("tag", [t for t, _ in GEN.FEAT_CASES])
def test_features_match_the_reference(fx, narrow, gpu_device, tag):
    from movae_amd import metrics

    x = GEN.raw_images(int(fx[f"feat.{tag}.seed"]), tuple(int(v) for v in fx[f"feat.{tag}.shape"]))
    got = metrics.inception_features(x.to(gpu_device))
    within(got, fx[f"feat.{tag}.f64"], fx[f"feat.{tag}.f32"], f"features {tag}")
    if tag == "32x32":  # per-sample features do not depend on how the set is cut into chunks
        assert torch.equal(metrics.inception_features(x.to(gpu_device), chunk=1), got)
        assert torch.equal(metrics.inception_features(x.to(gpu_device), chunk=2), got)


@pytest.mark.gpu
def test_fid_matches_the_reference(fx, narrow, gpu_device):
    """FID of the fixture's two sets against the reference's float64 value; bound: 4 x the fixture's yardstick (the largest
    deviation of the reference's two float32 CPU runs from its float64 run)."""
    from movae_amd import metrics

    real, fake = GEN.fid_sets(int(fx["fid.seed"]), int(fx["fid.n"]), int(fx["fid.side"]))
    got = metrics.fid(real.to(gpu_device), fake.to(gpu_device))
    truth, yard = float(fx["fid.f64"]), float(fx["fid.yardstick"])
    print(f"fid {got!r}, float64 reference {truth!r}, error {abs(got - truth):.3e}, yardstick {yard:.3e}, ratio {abs(got - truth) / yard:.2f}")
    assert abs(got - truth) <= 4 * yard
    # what the bound tells apart (recorded by the generator): the plain a = -0.75 resize and a missing 0.5 x + 0.5
    assert min(abs(float(fx["fid.no_antialias"]) - truth), abs(float(fx["fid.no_denorm"]) - truth)) > 40 * yard
    assert math.isnan(metrics.fid(real[:0].to(gpu_device), fake.to(gpu_device)))


@pytest.mark.gpu
def test_accumulator_rfid_equals_fid_of_the_concatenation(fx, narrow, gpu_device):
    from movae_amd import metrics

    real, fake = (t[:70].to(gpu_device) for t in GEN.fid_sets(int(fx["fid.seed"]), 80, 32))
    whole = metrics.fid(real, fake)
    acc = metrics.ReconMetricAccumulator(gpu_device, 70, chunk=32)
    lo = 0
    for n in (5, 40, 1, 30):  # uneven batches, the last one cut at max_samples
        acc.add(real[lo: lo + n], fake[lo: lo + n])
        lo += n
    res = acc.result()
    print(f"accumulated rfid {res['rfid']!r}, fid of the concatenation {whole!r}")
    assert acc.count == 70 and math.isfinite(whole) and whole > 0
    assert abs(res["rfid"] - whole) <= 1e-9 * whole
    assert math.isfinite(res["ssim"]) and math.isfinite(res["psnr"]) and math.isnan(res["lpips"])
    # the reference's gates: the width (min_size_for_lpips), n >= 2, 3 channels
    for shape, cap in (((8, 3, 16, 16), 8), ((1, 3, 32, 32), 1), ((8, 1, 32, 32), 8)):
        acc = metrics.ReconMetricAccumulator(gpu_device, cap, chunk=32)
        acc.add(torch.rand(shape, device=gpu_device), torch.rand(shape, device=gpu_device))
        res = acc.result()
        assert math.isnan(res["rfid"]) and math.isfinite(res["psnr"]), shape


@pytest.mark.gpu
def test_training_run_reports_rfid(fx, narrow, gpu_device, tmp_path, capsys):
    from movae_amd import train

    argv = ["--dataset", "synthetic_cifar10", "--arch", "vae", "--agg", "upgrad", "--batch_size", "50", "--max_items", "500",
            "--latent_dim", "16", "--hidden_dims", "16", "32", "--save_path", str(tmp_path), "--seed", "2", "--device", "cuda:0",
            "--graph", "off", "--epochs", "1", "--eval_freq", "0", "--max_fid_samples", "128"]

    def run():
        args = train.parse_args(argv)
        train.set_seed(args.seed)
        train.main(args)
        final = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("final: ")]
        assert len(final) == 1
        return final[0], train.LAST_FINAL["recon"]

    line, rec = run()
    assert math.isfinite(rec["rfid"]) and rec["rfid"] > 0 and math.isfinite(rec["psnr"])
    m = re.search(r"rfid: ([-+0-9.eE]+)", line)
    assert m and float(m.group(1)) == pytest.approx(rec["rfid"], abs=1e-5)
    narrow.use_inception_weights(None)
    line, rec = run()
    assert math.isnan(rec["rfid"]) and re.search(r"rfid: nan", line)

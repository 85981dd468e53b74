"""The perceptual (VGG16 feature) loss (movae_amd/perceptual.py, csrc/perceptual.hip): the weight registry, loaders and refusals on the
CPU; on the GPU the two kernel pairs against torch float64, PerceptualLoss against vectors recorded from the reference's own class
around a narrow stack (tests/golden/generate_perceptual.py) and against a torch composition at the real VGG16 widths, and both Sphere
Encoders with use_perceptual=True (losses, Jacobian rows, aggregated and summed step, Adam step, graph replay).

Tolerance rule of the fixture comparisons: the truth is the reference in fp64; the bound is 4 x the deviation of the reference's own fp32
run from it for that quantity (the 4 covers the other summation order of the tiled kernels), and never tighter than the tolerances
tests/test_sphere_encoder.py holds the same quantity to."""
import ast

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, meta_of

CONVS = (0, 2, 5, 7, 10, 12, 14)
KEYS = [f"features.{n}.{leaf}" for n in CONVS for leaf in ("weight", "bias")]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


class Args:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def T(a):
    return torch.from_numpy(np.asarray(a))


def narrow_weights():
    fx = load_golden("perceptual_tiny")
    return {k: T(fx["vgg." + k]) for k in KEYS}


@pytest.fixture
def registry(monkeypatch):
    """The module's registry, empty at the start and emptied at the end, and no environment fallback."""
    import movae_amd  # noqa: F401
    from movae_amd import perceptual

    monkeypatch.delenv(perceptual.ENV_VAR, raising=False)
    perceptual.use_vgg16_weights(None)
    yield perceptual
    perceptual.use_vgg16_weights(None)


def bounded(got, truth, yard, what, rtol, atol):
    """|got - truth| <= max(4 |yard - truth|_max, rtol |truth| + atol max(1, |truth|_max)) element-wise; prints the figures first."""
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    truth, yard = np.asarray(truth, dtype=np.float64), np.asarray(yard, dtype=np.float64)
    dev = float(np.abs(yard - truth).max())
    err = np.abs(got - truth)
    allow = np.maximum(4 * dev, rtol * np.abs(truth) + atol * max(1.0, float(np.abs(truth).max())))
    print(f"{what}: error {float(err.max()):.3g}, reference-fp32 deviation {dev:.3g}, |truth| max {float(np.abs(truth).max()):.3g}")
    assert (err <= allow).all(), f"{what}: error {float(err.max()):.3g} exceeds the bound {float(np.max(allow)):.3g} (4 x {dev:.3g} or the floor)"


# ---- CPU: registry, loaders, refusals ---------------------------------------------------------------------------------------------
VIT_KW = dict(img_size=8, patch_size=2, embed_dim=16, depth=1, num_heads=2, mixer_depth=1, mixer_tokens_mlp_dim=8, mixer_channels_mlp_dim=16,
              latent_channels=2)


def test_registry_gates_both_models_and_the_objective_factory(registry):
    from movae_amd import objectives
    from movae_amd.models import SphereEncoder, SphereEncoderViT

    def refused():
        with pytest.raises(NotImplementedError, match="VGG16"):
            SphereEncoder(latent_dim=6, hidden_dims=[4, 8], input_size=16)
        with pytest.raises(NotImplementedError, match="VGG16"):
            SphereEncoderViT(**VIT_KW)
        with pytest.raises(NotImplementedError, match="VGG16"):
            objectives.get_recon_obj_and_activation("perceptual", None, model=torch.nn.Module())

    refused()
    assert registry.registered_vgg16_weights() is None
    registry.use_vgg16_weights(narrow_weights())
    for net in (SphereEncoder(latent_dim=6, hidden_dims=[4, 8], input_size=16), SphereEncoderViT(**VIT_KW)):
        assert net.use_perceptual and isinstance(net.perceptual_loss, registry.PerceptualLoss)
        keys = list(net.state_dict().keys())
        assert keys[-len(KEYS):] == ["perceptual_loss." + k for k in KEYS]  # the last submodule, as in the reference
        assert all(p.requires_grad is False for p in net.perceptual_loss.parameters())
        assert all(p.requires_grad for n, p in net.named_parameters() if not n.startswith("perceptual_loss."))
        net.train()
        assert net.training and not net.perceptual_loss.training and not net.perceptual_loss.features.training
    host = torch.nn.Module()
    fn, act = objectives.get_recon_obj_and_activation("perceptual", None, model=host)
    assert act == "tanh" and callable(fn) and list(host.state_dict().keys()) == ["perceptual_loss." + k for k in KEYS]
    assert objectives.get_recon_obj_and_activation("perceptual", "sigmoid", model=torch.nn.Module())[1] == "sigmoid"
    with pytest.raises(ValueError, match="model required"):
        objectives.get_recon_obj_and_activation("perceptual", None)
    registry.use_vgg16_weights(None)
    refused()


def test_state_dict_matches_the_fixture_and_is_frozen(registry):
    fx = load_golden("perceptual_tiny")
    assert [f[4:] for f in fx.files if f.startswith("vgg.")] == KEYS
    pl = registry.PerceptualLoss(narrow_weights())
    sd = pl.state_dict()
    assert list(sd.keys()) == KEYS
    for k in KEYS:
        assert np.array_equal(sd[k].numpy(), fx["vgg." + k]), k
    assert all(p.requires_grad is False for p in pl.parameters()) and not pl.training
    assert pl.train() is pl and not pl.training and not pl.features.training
    # a reference checkpoint's keys load into a model built on other weights
    from movae_amd.models import SphereEncoder

    registry.use_vgg16_weights({k: torch.zeros_like(v) for k, v in narrow_weights().items()})
    net = SphereEncoder(latent_dim=6, hidden_dims=[4, 8], input_size=16)
    ref = load_golden("sphere_encoder_tiny_perceptual")
    want = [f[4:] for f in ref.files if f.startswith("sd0.")]
    assert [k for k in want if k.startswith("perceptual_loss.")] == ["perceptual_loss." + k for k in KEYS]
    net.perceptual_loss.load_state_dict({k[len("perceptual_loss."):]: T(ref["sd0." + k]) for k in want if k.startswith("perceptual_loss.")})
    assert np.array_equal(net.state_dict()["perceptual_loss.features.14.weight"].numpy(), fx["vgg.features.14.weight"])
    assert all(p.requires_grad is False for p in net.perceptual_loss.parameters())


def test_default_widths_are_vgg16s():
    import movae_amd  # noqa: F401
    from movae_amd.perceptual import PerceptualLoss

    torch.manual_seed(0)
    pl = PerceptualLoss()
    shapes = [tuple(v.shape) for k, v in pl.state_dict().items() if k.endswith("weight")]
    assert shapes == [(64, 3, 3, 3), (64, 64, 3, 3), (128, 64, 3, 3), (128, 128, 3, 3), (256, 128, 3, 3), (256, 256, 3, 3), (256, 256, 3, 3)]
    assert "NOT the pretrained network" in PerceptualLoss.__doc__


def test_loader_key_spellings_and_errors(registry, tmp_path):
    w = narrow_weights()
    full = dict(w)  # a full torchvision state_dict: later feature layers and the classifier are ignored
    full.update({"features.17.weight": torch.zeros(4, 32, 3, 3), "features.17.bias": torch.zeros(4), "classifier.0.weight": torch.zeros(2, 2)})
    forms = [full, {k[len("features."):]: v for k, v in w.items()}, {"perceptual_loss." + k: v for k, v in w.items()}]
    path = tmp_path / "vgg.pt"
    torch.save(w, path)
    forms.append(str(path))
    for src in forms:
        got = registry.load_vgg16_weights(src)
        assert list(got.keys()) == KEYS and all(torch.equal(got[k], w[k]) for k in KEYS)
    bad = dict(w)
    bad["features.5.weight"] = torch.zeros(16, 7, 3, 3)
    with pytest.raises(ValueError, match=r"features\.5\.weight"):
        registry.load_vgg16_weights(bad)
    with pytest.raises(ValueError, match=r"features\.5\.weight"):
        registry.use_vgg16_weights(bad)
    assert registry.registered_vgg16_weights() is None
    bad = dict(w)
    bad["features.7.bias"] = torch.zeros(15)
    with pytest.raises(ValueError, match=r"features\.7\.bias"):
        registry.load_vgg16_weights(bad)
    missing = {k: v for k, v in w.items() if k != "features.12.bias"}
    with pytest.raises(ValueError, match=r"features\.12\.bias"):
        registry.load_vgg16_weights(missing)
    odd = dict(w)  # the convolution in front of a pool must have Cout % 4 == 0
    odd["features.2.weight"], odd["features.2.bias"], odd["features.5.weight"] = torch.zeros(6, 8, 3, 3), torch.zeros(6), torch.zeros(16, 6, 3, 3)
    with pytest.raises(ValueError, match=r"features\.2\.weight"):
        registry.load_vgg16_weights(odd)


def test_environment_variable_is_the_fallback(registry, tmp_path, monkeypatch):
    from movae_amd.models import SphereEncoder

    path = tmp_path / "vgg.pt"
    torch.save(narrow_weights(), path)
    monkeypatch.setenv(registry.ENV_VAR, str(path))
    net = SphereEncoder(latent_dim=6, hidden_dims=[4, 8], input_size=16)
    assert net.use_perceptual and net.perceptual_loss.state_dict()["features.0.weight"].shape == (8, 3, 3, 3)
    registry.use_vgg16_weights({k: v * 2 for k, v in narrow_weights().items()})  # a registration wins over the environment
    net2 = SphereEncoder(latent_dim=6, hidden_dims=[4, 8], input_size=16)
    assert torch.equal(net2.perceptual_loss.state_dict()["features.0.bias"], 2 * net.perceptual_loss.state_dict()["features.0.bias"])


# ---- GPU: vgg_prep ------------------------------------------------------------------------------------------------------------------
def _prep_ref(x64):
    """PerceptualLoss._norm_input (utils/objectives.py:66-72) on an NHWC float64 tensor."""
    x = x64
    if x.min() < 0:
        x = (x + 1) / 2
    x = torch.clamp(x, 0, 1)
    return (x - torch.tensor(MEAN, dtype=x.dtype)) / torch.tensor(STD, dtype=x.dtype)


def _off_edges(x, rescaled):
    """Moves every element at least 1e-3 (in the clamped variable) away from the clamp edges 0 and 1."""
    xp = (x + 1) / 2 if rescaled else x
    for edge in (0.0, 1.0):
        near = (xp - edge).abs() < 2e-3
        xp = torch.where(near, xp + 4e-3, xp)
    return xp * 2 - 1 if rescaled else xp


def _prep_cases(shape, seed):
    g = torch.Generator().manual_seed(seed)
    u = lambda: torch.rand(shape, generator=g)  # noqa: E731
    cases = {"negatives": _off_edges(u() * 1.9 - 0.95, True), "unit": u() * 0.9 + 0.05,
             "rescaled_clamped": _off_edges(u() * 3.0 - 1.5, True), "clamped": _off_edges(u() * 1.45 + 0.05, False)}
    cases["unit"][0, 0, 0, 0] = 0.05
    assert cases["negatives"].min() < 0 and cases["rescaled_clamped"].min() < 0 and cases["unit"].min() >= 0.05 and cases["unit"].max() <= 0.95
    assert cases["clamped"].min() > 0 and cases["clamped"].max() > 1
    return cases


PREP_SHAPES = [(3, 5, 7, 3), (2, 8, 8, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", PREP_SHAPES)
def test_vgg_prep_against_float64(shape, gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import ops

    cases = _prep_cases(shape, 31 + shape[1])
    cot = torch.randn(shape, generator=torch.Generator().manual_seed(5))
    want = {}
    for name, x in cases.items():
        x64 = x.double().requires_grad_(True)
        y64 = _prep_ref(x64)
        want[name] = (y64.detach(), torch.autograd.grad(y64, x64, cot.double())[0])
        xd = x.to(gpu_device).requires_grad_(True)
        y = ops.vgg_prep(xd)
        dx = torch.autograd.grad(y, xd, cot.to(gpu_device))[0]
        torch.testing.assert_close(y.detach().cpu().double(), want[name][0], rtol=1e-5, atol=1e-6, msg=lambda m: f"{name} forward: {m}")
        torch.testing.assert_close(dx.cpu().double(), want[name][1], rtol=1e-5, atol=1e-6, msg=lambda m: f"{name} backward: {m}")
        out_of_range = ((x + 1) / 2 if x.min() < 0 else x)
        dead = (out_of_range < 0) | (out_of_range > 1)
        assert bool((dx.cpu()[dead] == 0).all()), f"{name}: a clamped element has a non-zero gradient"
        if "clamped" in name:
            assert int(dead.sum()) > 0
        with torch.no_grad():  # nothing is saved, the values are the same
            assert torch.equal(ops.vgg_prep(xd), y.detach())
    # a grouped call whose members take different branches: two launches for all, each member as in its own call
    names = list(cases)
    xs = [cases[n].to(gpu_device).requires_grad_(n != "unit") for n in names]
    ys = ops.vgg_prep(*xs)
    assert len(ys) == len(names) and not ys[names.index("unit")].requires_grad
    for n, y in zip(names, ys):
        torch.testing.assert_close(y.detach().cpu().double(), want[n][0], rtol=1e-5, atol=1e-6, msg=lambda m: f"grouped {n}: {m}")
    live = [i for i, n in enumerate(names) if n not in ("unit", "clamped")]  # only some cotangents arrive
    gs = torch.autograd.grad([ys[i] for i in live], [xs[i] for i in live], [cot.to(gpu_device)] * len(live))
    for i, gx in zip(live, gs):
        torch.testing.assert_close(gx.cpu().double(), want[names[i]][1], rtol=1e-5, atol=1e-6, msg=lambda m: f"grouped backward {names[i]}: {m}")


# ---- GPU: max-pool -----------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(2, 8, 8, 64), (1, 6, 10, 4), (1, 7, 5, 8)]


def _torch_pool(x_nhwc, dy_nhwc):
    x = x_nhwc.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.max_pool2d(x, kernel_size=2, stride=2)
    dx = torch.autograd.grad(y, x, dy_nhwc.permute(0, 3, 1, 2))[0]
    return y.detach().permute(0, 2, 3, 1), dx.permute(0, 2, 3, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_max_pool_equals_torch_exactly(shape, gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import ops

    n, h, w, c = shape
    g = torch.Generator().manual_seed(h * w + c)
    x = (torch.randperm(n * h * w * c, generator=g).float() - 1000.0).reshape(shape)  # distinct values: no ties
    dy = torch.randn(n, h // 2, w // 2, c, generator=g)
    y_want, dx_want = _torch_pool(x, dy)
    xd = x.to(gpu_device).requires_grad_(True)
    y = ops.max_pool2x2(xd)
    assert y.shape == (n, h // 2, w // 2, c) and torch.equal(y.detach().cpu(), y_want)
    dx = torch.autograd.grad(y, xd, dy.to(gpu_device))[0].cpu()
    assert torch.equal(dx, dx_want)
    if h % 2:
        assert bool((dx[:, h - 1] == 0).all())
    if w % 2:
        assert bool((dx[:, :, w - 1] == 0).all())
    with torch.no_grad():
        assert torch.equal(ops.max_pool2x2(xd).cpu(), y_want)


@pytest.mark.gpu
def test_max_pool_ties_after_relu(gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import ops

    n, h, w, c = 2, 7, 6, 8
    g = torch.Generator().manual_seed(3)
    x = torch.relu(torch.randn(n, h, w, c, generator=g))
    x[:, 0:2, 0:2] = 0.0  # whole-zero windows
    x[:, 2:4, 2:6, :4] = 0.0
    dy = torch.randint(1, 9, (n, h // 2, w // 2, c), generator=g).float()  # integers: the sums below are exact
    y_want, dx_want = _torch_pool(x, dy)
    xd = x.to(gpu_device).requires_grad_(True)
    y = ops.max_pool2x2(xd)
    dx = torch.autograd.grad(y, xd, dy.to(gpu_device))[0].cpu()
    assert torch.equal(y.detach().cpu(), y_want) and torch.equal(dx, dx_want)
    win = dx[:, : 2 * (h // 2), : 2 * (w // 2)].reshape(n, h // 2, 2, w // 2, 2, c)
    hits = (win != 0).sum(dim=(2, 4))
    assert bool((hits == 1).all()), "a window's dy must land on exactly one element"
    assert torch.equal(win.sum(dim=(2, 4)), dy) and float(dx.sum()) == float(dy.sum())
    assert bool((win[:, 0, 0, 0, 0] == dy[:, 0, 0]).all())  # an all-zero window: the first element in scan order takes it


# ---- GPU: PerceptualLoss ---------------------------------------------------------------------------------------------------------------
#: tests/test_sphere_encoder.py assert_close defaults, the floor of every fixture comparison here
FLOOR = dict(rtol=1e-3, atol=3e-6)


@pytest.mark.gpu
def test_perceptual_loss_against_the_reference_fixture(gpu_device):
    """Figures on an MI355X (error against fp64 / the reference's own fp32 deviation): see the printed lines; the bound is
    max(4 x deviation, floor)."""
    import movae_amd  # noqa: F401
    from movae_amd.perceptual import PerceptualLoss

    fx = load_golden("perceptual_tiny")
    pl = PerceptualLoss(narrow_weights(), device=gpu_device)
    before = {k: v.clone() for k, v in pl.state_dict().items()}
    for tag in [str(s) for s in fx["cases"]]:
        pred = T(fx[f"{tag}.pred"]).to(gpu_device).requires_grad_(True)
        target = T(fx[f"{tag}.target"]).to(gpu_device)
        loss = pl(pred, target)
        grad = torch.autograd.grad(loss, pred)[0]
        bounded(loss, fx[f"{tag}.loss.f64"], fx[f"{tag}.loss.f32"], f"{tag} loss", **FLOOR)
        bounded(grad, fx[f"{tag}.grad.f64"], fx[f"{tag}.grad.f32"], f"{tag} d loss / d pred", **FLOOR)
        with torch.no_grad():
            torch.testing.assert_close(pl(pred, target), loss.detach(), rtol=1e-6, atol=0)
        # features_of + feature_mse is the same computation in pieces
        pieces = pl.feature_mse(pl.features_of(pred), pl.features_of(target))
        torch.testing.assert_close(pieces.detach(), loss.detach(), rtol=1e-6, atol=0)
    assert all(torch.equal(v, before[k]) for k, v in pl.state_dict().items())


def _torch_perceptual(sd, pred, target, dtype):
    """The reference's forward as a torch composition in `dtype` on the CPU -> (loss, d loss / d pred)."""
    def norm(x):
        if x.min() < 0:
            x = (x + 1) / 2
        x = torch.clamp(x, 0, 1)
        return (x - torch.tensor(MEAN, dtype=dtype).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=dtype).view(1, 3, 1, 1)

    def feats(x):
        for n in CONVS:
            x = F.relu(F.conv2d(x, sd[f"features.{n}.weight"].to(dtype), sd[f"features.{n}.bias"].to(dtype), padding=1))
            if n in (2, 7):
                x = F.max_pool2d(x, 2, 2)
        return x

    p = pred.to(dtype).requires_grad_(True)
    loss = F.mse_loss(feats(norm(p)), feats(norm(target.to(dtype))))
    return loss.detach(), torch.autograd.grad(loss, p)[0]


@pytest.mark.gpu
def test_perceptual_loss_at_the_real_widths(gpu_device):
    """The dispatcher coverage of the real VGG16 shapes (3 -> 64 ... 256 -> 256, and the 64 -> 3 input gradient) on 2x3x8x8."""
    import movae_amd  # noqa: F401
    from movae_amd.perceptual import PerceptualLoss

    torch.manual_seed(1234)
    pl = PerceptualLoss()
    sd = {k: v.clone() for k, v in pl.state_dict().items()}
    for k in sd:  # torch's default init makes features of order 1e-3: scale the weights so the loss is of order one
        if k.endswith("weight"):
            sd[k] = sd[k] * 3.0
    pl.load_state_dict(sd)
    pl = pl.to(gpu_device)
    g = torch.Generator().manual_seed(9)
    pred = torch.rand(2, 3, 8, 8, generator=g) * 1.9 - 0.95
    target = torch.rand(2, 3, 8, 8, generator=g) * 0.9 + 0.05
    l64, g64 = _torch_perceptual(sd, pred, target, torch.float64)
    l32, g32 = _torch_perceptual(sd, pred, target, torch.float32)
    pd = pred.to(gpu_device).requires_grad_(True)
    loss = pl(pd, target.to(gpu_device))
    grad = torch.autograd.grad(loss, pd)[0]
    assert float(l64) > 1e-4
    bounded(loss, l64.numpy(), l32.numpy(), "full-width loss", **FLOOR)
    bounded(grad, g64.numpy(), g32.numpy(), "full-width d loss / d pred", **FLOOR)


# ---- GPU: the Sphere Encoders with the term ------------------------------------------------------------------------------------------
MODEL_TAG = "sphere_encoder_tiny_perceptual"
AGG = dict(agg_norm_eps=1e-4, agg_reg_eps=1e-4, mgda_epsilon=1e-5, mgda_max_iters=250, pref_weights=None)


def _model(registry, dev):
    from movae_amd.models import SphereEncoder

    fx = load_golden(MODEL_TAG)
    m = meta_of(fx)
    registry.use_vgg16_weights({k: T(fx["sd0.perceptual_loss." + k]) for k in KEYS})
    torch.manual_seed(int(m["seed"]))
    net = SphereEncoder(latent_dim=int(m["latent_dim"]), hidden_dims=ast.literal_eval(m["hidden_dims"]), input_size=int(m["input_size"]),
                        in_channels=3, recons_objective=m["objective"], recons_activation=None, lambda_weights=[1.0, 0.0])
    sd0 = [f[4:] for f in fx.files if f.startswith("sd0.")]
    assert list(net.state_dict().keys()) == sd0
    for k in sd0:
        assert np.array_equal(net.state_dict()[k].numpy(), fx["sd0." + k]), f"init replay {k}"
    net = net.to(dev).train()
    net.noise_override = {"u": T(fx["u"]).to(dev), "e": T(fx["e"]).to(dev)}
    return net, fx


def _vgg_snapshot(net):
    return {k: v.clone() for k, v in net.perceptual_loss.state_dict().items()}


@pytest.mark.gpu
def test_model_losses_jacobian_rows_and_adam_step(registry, gpu_device):
    from movae_amd import train

    net, fx = _model(registry, gpu_device)
    vgg0 = _vgg_snapshot(net)
    x = T(fx["x"]).to(gpu_device)
    out = net(x)
    for k in ("recons", "x_recon_NOISY", "v_enc_dec"):
        bounded(out[k], fx["f64.out." + k], fx["out." + k], k, rtol=2e-4, atol=2e-5)
    ld = net.loss_function(x, args=out)
    assert list(ld.keys()) == ["pix_recon", "pix_con", "lat_con", "total_loss"]
    for k, v in ld.items():
        bounded(v, fx["f64.loss." + k], fx["loss." + k], "loss " + k, rtol=2e-5, atol=1e-7)
    # the term is there: without it pix_recon is sphere_encoder_tiny's
    plain = load_golden("sphere_encoder_tiny")
    assert float(fx["loss.pix_recon"]) > float(plain["loss.pix_recon"]) * 1.01
    named = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
    assert [n for n, _ in named] == [f[len("gsum."):] for f in fx.files if f.startswith("gsum.")]
    comp = [v for k, v in ld.items() if k != "total_loss"]
    for i, v in enumerate(comp):
        gs = torch.autograd.grad(v, [p for _, p in named], retain_graph=True, allow_unused=True)
        for (n, _), gr in zip(named, gs):
            assert gr is not None, f"row {i} leaves {n} without a gradient"
            bounded(gr, fx[f"f64.gloss.{i}.{n}"], fx[f"gloss.{i}.{n}"], f"row {i} {n}", rtol=2e-3, atol=1e-5)
    # the summed step through train.forward_backward and FusedAdam (the frozen VGG tensors sit in net.parameters())
    a = Args(aggregator="sum", optimizer="adam", lr=1e-3, wd=0, momentum=0.9, max_grad_norm=None, **AGG)
    net2, _ = _model(registry, gpu_device)
    opt = train.make_optimizer(net2, a)
    train.forward_backward(net2, x, opt, "sum")
    for n, p in net2.named_parameters():
        if not p.requires_grad:
            assert p.grad is None, n
            continue
        bounded(p.grad, fx["f64.gsum." + n], fx["gsum." + n], "grad " + n, **FLOOR)
    opt.step()
    sd1 = net2.state_dict()
    for k in [f[4:] for f in fx.files if f.startswith("sd1.")]:
        if k.endswith("num_batches_tracked"):
            assert int(sd1[k].item()) == int(fx["sd1." + k]) == 2, k
            continue
        noise = ("gsum." + k) in fx.files and np.abs(fx["gsum." + k]).max() < 1e-6
        bounded(sd1[k], fx["f64.sd1." + k], fx["sd1." + k], "after Adam " + k, rtol=2e-4, atol=2.1e-3 if noise else 3e-5)
    for nn_ in (net, net2):
        assert all(torch.equal(v, vgg0[k]) for k, v in nn_.perceptual_loss.state_dict().items()), "the VGG tensors changed"
    assert not any(id(p) in {id(q) for q in net2.perceptual_loss.parameters()} for p in opt.state)


@pytest.mark.gpu
def test_model_upgrad_step_matches_oracle_on_fixture_jacobian(registry, gpu_device):
    from movae_amd import aggregation, train
    from oracle.aggregation import aggregate, make_weighting

    net, fx = _model(registry, gpu_device)
    named = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
    K = 3
    J = torch.cat([torch.cat([T(fx[f"f64.gloss.{i}.{n}"]).reshape(-1) for n, _ in named]).reshape(1, -1) for i in range(K)]).double()
    losses = np.array([float(fx["f64.loss." + k]) for k in ("pix_recon", "pix_con", "lat_con")])
    g_want, w_want, _ = aggregate(J, make_weighting("upgrad"), losses)
    A = aggregation.make_aggregator(Args(aggregator="upgrad", **AGG))
    seen = {}
    A.weighting.register_forward_hook(lambda mod, inp, out: seen.update(w=out.clone()))
    x = T(fx["x"]).to(gpu_device)
    train.forward_backward(net, x, torch.optim.SGD([p for _, p in named], lr=0.0), A)
    np.testing.assert_allclose(seen["w"].cpu().numpy(), w_want.numpy(), rtol=1e-3, atol=1e-4)
    off = 0
    for n, p in named:  # tests/test_sphere_encoder.py holds the aggregated gradient to rtol 2e-3, atol 1e-5 of the scale
        want = g_want[off: off + p.numel()].reshape(p.shape).numpy()
        off += p.numel()
        got = p.grad.detach().cpu().double().numpy()
        np.testing.assert_allclose(got, want, rtol=2e-3, atol=1e-5 * max(1.0, float(np.abs(want).max())), err_msg=f"upgrad grad {n}")
    assert all(p.grad is None for p in net.perceptual_loss.parameters())


@pytest.mark.gpu
def test_graph_replay_matches_the_eager_step(registry, gpu_device):
    from movae_amd import aggregation
    from movae_amd.train import GraphedTrainStep, make_optimizer, train_step

    a = Args(aggregator="upgrad", optimizer="adam", lr=1e-3, wd=0, momentum=0.9, max_grad_norm=None, **AGG)
    net_e, fx = _model(registry, gpu_device)
    x = T(fx["x"]).to(gpu_device)
    opt_e, agg_e = make_optimizer(net_e, a, capturable=True), aggregation.make_aggregator(a)
    eager = [{k: v.item() for k, v in train_step(net_e, x, opt_e, agg_e, a)[0].items()} for _ in range(2)]
    net_g, _ = _model(registry, gpu_device)
    vgg0 = _vgg_snapshot(net_g)
    gs = GraphedTrainStep(net_g, make_optimizer(net_g, a, capturable=True), aggregation.make_aggregator(a), a, x, preserve_state=True)
    assert net_g.noise_override is not None
    graphed = [{k: v.item() for k, v in gs.step(x)[0].items()} for _ in range(2)]
    for k in eager[0]:
        bounded(eager[0][k], fx["f64.loss." + k], fx["loss." + k], "eager step 1 " + k, rtol=2e-5, atol=1e-7)
        # (tests/test_sphere_encoder.py: a replay equals the eager step to rtol 2e-5)
        np.testing.assert_allclose([s[k] for s in graphed], [s[k] for s in eager], rtol=2e-5, atol=1e-7, err_msg=k)
    assert all(torch.equal(v, vgg0[k]) for k, v in net_g.perceptual_loss.state_dict().items())


@pytest.mark.gpu
def test_vit_takes_a_step_with_the_term(registry, gpu_device):
    from movae_amd import aggregation, train
    from movae_amd.models import SphereEncoderViT

    registry.use_vgg16_weights(narrow_weights())
    m = meta_of(load_golden("sphere_encoder_vit_tiny"))
    torch.manual_seed(0)
    net = SphereEncoderViT(**ast.literal_eval(m["kwargs"])).to(gpu_device).train()  # use_perceptual defaults to True
    assert net.use_perceptual
    a = Args(aggregator="upgrad", optimizer="adam", lr=1e-3, wd=0, momentum=0.9, max_grad_norm=1.0, **AGG)
    opt, A = train.make_optimizer(net, a), aggregation.make_aggregator(a)
    x = torch.rand(int(m["B"]), 3, net.img_size, net.img_size, generator=torch.Generator().manual_seed(1)).to(gpu_device)
    before = net.head_dec.weight.detach().clone()
    ld, _ = train.forward_backward(net, x, opt, A)
    assert list(ld.keys()) == ["pix_recon", "pix_con", "lat_con", "total_loss"] and all(np.isfinite(v.item()) for v in ld.values())
    gw = net.head_dec.weight.grad
    assert gw is not None and bool(torch.isfinite(gw).all()) and float(gw.abs().max()) > 0
    opt.step()
    assert not torch.equal(net.head_dec.weight.detach(), before) and all(p.grad is None for p in net.perceptual_loss.parameters())
    # with the term's weights at zero the loss_function is the plain one
    net.pix_recon_perceptual_weight = net.pix_con_perceptual_weight = 0.0
    with torch.no_grad():
        out = net(x)
        plain = net.loss_function(x, args=out)
        net.pix_recon_perceptual_weight = 1.0
        with_term = net.loss_function(x, args=out)
    assert with_term["pix_recon"].item() > plain["pix_recon"].item()
    np.testing.assert_allclose(with_term["pix_con"].item(), plain["pix_con"].item(), rtol=1e-6)

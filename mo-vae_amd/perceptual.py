"""The reference's PerceptualLoss (utils/objectives.py:53-79, models/sphere_encoder.py:46-72) on the HIP kernels: a frozen VGG16 feature
stack up to relu3_3 (`vgg16.features[:16]`: seven 3x3 stride-1 convolutions with ReLU, two 2x2 max-pools), a data-dependent input
normalisation in front (ops.vgg_prep) and an MSE on the features behind (ops.recon_loss).  The convolutions are ops.conv2d with the ReLU
in their epilogue; the weights are frozen, so the backward runs the input-gradient kernels alone.

This build fetches no weights.  The caller registers the ones they already have -- `use_vgg16_weights(path or mapping)`, or the environment
variable MOVAE_VGG16_WEIGHTS=/path as the fallback -- and the Sphere Encoders' `use_perceptual=True` and
objectives.get_recon_obj_and_activation("perceptual") then build; with nothing registered they refuse as before.

The same registration serves the LPIPS metric (metrics.lpips; the reference's utils/metrics.py:206-357): when the source also holds the
conv4 block, features.{17,19,21}, `registered_vgg16_lpips_weights()` returns the twenty tensors of the ten convolutions up to relu4_3
and `LpipsFeatures` is the stack that taps relu1_2, relu2_2, relu3_3 and relu4_3."""
import os
from collections import OrderedDict

import torch
import torch.nn as tnn

from . import ops

#: torchvision's indices of the convolutions in vgg16.features[:16]; ReLU sits at the odd gaps, the pools at 4 and 9
CONV_INDICES = (0, 2, 5, 7, 10, 12, 14)
#: a 2x2 max-pool follows these convolutions (+ ReLU)
POOL_AFTER = (2, 7)
VGG16_WIDTHS = (64, 64, 128, 128, 256, 256, 256)
#: the conv4 block the LPIPS metric adds behind a third pool (metrics.lpips; the reference's utils/metrics.py:206-282 VGGFeatureExtractor)
LPIPS_EXTRA_INDICES = (17, 19, 21)
LPIPS_CONV_INDICES = CONV_INDICES + LPIPS_EXTRA_INDICES
LPIPS_POOL_AFTER = POOL_AFTER + (14,)
#: the metric's taps relu1_2, relu2_2, relu3_3, relu4_3 (torchvision's 3, 8, 15, 22), named by the convolution in front of each ReLU
LPIPS_TAP_AFTER = (2, 7, 14, 21)
LPIPS_VGG16_WIDTHS = VGG16_WIDTHS + (512, 512, 512)
ENV_VAR = "MOVAE_VGG16_WEIGHTS"
_PREFIXES = ("perceptual_loss.features.", "features.", "")

_registered = [None]


def _open(src):
    """A path (read with torch.load(..., weights_only=True)), a module or a checkpoint -> the mapping that holds the tensors."""
    if isinstance(src, (str, os.PathLike)):
        src = torch.load(os.fspath(src), map_location="cpu", weights_only=True)
    if hasattr(src, "state_dict") and not hasattr(src, "keys"):
        src = src.state_dict()
    if isinstance(src, dict) and "state_dict" in src and not any(str(k).endswith(".weight") for k in src):
        src = src["state_dict"]
    return src


def _find(src, n, leaf):
    return next((p + f"{n}.{leaf}" for p in _PREFIXES if p + f"{n}.{leaf}" in src), None)


def _take(src, indices, cin, pool_after, out):
    """Validates the convolutions `indices` of the mapping, chained from `cin` input channels, into out; -> the last width."""
    for n in indices:
        for leaf in ("weight", "bias"):
            key = f"features.{n}.{leaf}"
            found = _find(src, n, leaf)
            if found is None:
                raise ValueError(f"VGG16 weights: missing {key} (looked for {', '.join(p + f'{n}.{leaf}' for p in _PREFIXES)})")
            t = torch.as_tensor(src[found]).detach().to(device="cpu", dtype=torch.float32)
            if leaf == "weight":
                if t.dim() != 4 or tuple(t.shape[1:]) != (cin, 3, 3):
                    raise ValueError(f"VGG16 weights: {found} has shape {tuple(t.shape)}, expected [Cout, {cin}, 3, 3]")
                if n in pool_after and t.shape[0] % 4:
                    raise ValueError(f"VGG16 weights: {found} feeds a max-pool, so its Cout must be a multiple of 4 (got {t.shape[0]})")
                cin = t.shape[0]
            elif tuple(t.shape) != (cin,):
                raise ValueError(f"VGG16 weights: {found} has shape {tuple(t.shape)}, expected [{cin}]")
            out[key] = t
    return cin


def load_vgg16_weights(src):
    """-> OrderedDict {"features.N.weight" / "features.N.bias": fp32 CPU tensor} for N in CONV_INDICES, from a path (read with
    torch.load(..., weights_only=True)) or a mapping.  Accepted key forms: `features.N.*` (a full torchvision vgg16 state_dict: its
    classifier.* and later feature layers are ignored), `N.*`, and `perceptual_loss.features.N.*` (a reference checkpoint).  Any channel
    widths with the VGG topology are accepted, provided the convolutions feeding a pool have Cout % 4 == 0 (the pool kernel's access
    width).  A missing layer or a wrong shape raises ValueError naming the key."""
    out = OrderedDict()
    _take(_open(src), CONV_INDICES, 3, POOL_AFTER, out)
    return out


def load_vgg16_lpips_weights(src):
    """-> the 20-entry OrderedDict for N in LPIPS_CONV_INDICES (load_vgg16_weights' 14 entries, then features.{17,19,21}.*), or None
    when the source does not hold all six conv4 tensors (such a source stays valid for the loss).  Where it holds them they are
    validated like the others -- [Cout, Cin, 3, 3] chained from layer 14's width, which now feeds a pool: Cout % 4 == 0 -- and a
    wrong shape raises ValueError naming the key.  The metric needs no more of a width than the distance kernel: Cout % 4 == 0 at
    the four taps (layers 2, 7 and 14 feed pools; layer 21 is checked here)."""
    src = _open(src)
    if any(_find(src, n, leaf) is None for n in LPIPS_EXTRA_INDICES for leaf in ("weight", "bias")):
        return None
    out = OrderedDict()
    cin = _take(src, CONV_INDICES, 3, LPIPS_POOL_AFTER, out)
    _take(src, LPIPS_EXTRA_INDICES, cin, LPIPS_TAP_AFTER, out)
    return out


_registered_lpips = [None]
_env_loaded = [None]  # ((path, mtime_ns), 20-entry dict or None): the environment fallback's conv4 block is read once per file


def use_vgg16_weights(src):
    """Register the VGG16 weights of this process (a path or a mapping, validated now by load_vgg16_weights and, where the source
    holds the conv4 block, load_vgg16_lpips_weights); None removes the registration.  Every PerceptualLoss built afterwards copies
    them; metrics.lpips and the final evaluation use the 20-entry set."""
    if src is None:
        _registered[0] = _registered_lpips[0] = None
        return
    src = _open(src)
    base, ext = load_vgg16_weights(src), load_vgg16_lpips_weights(src)
    _registered[0], _registered_lpips[0] = base, ext


def registered_vgg16_weights():
    """The registered weights, else those at $MOVAE_VGG16_WEIGHTS, else None."""
    if _registered[0] is not None:
        return _registered[0]
    path = os.environ.get("MOVAE_VGG16_WEIGHTS")  # (ENV_VAR; spelled out: INTEGRATION.md's switch table is checked against the source)
    return load_vgg16_weights(path) if path else None


def registered_vgg16_lpips_weights():
    """The 20 entries of the ten convolutions up to relu4_3 from the same registration (else from $MOVAE_VGG16_WEIGHTS); None when
    nothing is registered or the source lacks the conv4 block.  The same object is returned until the registration (or the file
    behind the environment variable) changes: metrics.lpips keys its cached feature extractor on it."""
    if _registered[0] is not None:
        return _registered_lpips[0]
    path = os.environ.get(ENV_VAR)
    if not path:
        return None
    stamp = (path, os.stat(path).st_mtime_ns)
    if _env_loaded[0] is None or _env_loaded[0][0] != stamp:
        _env_loaded[0] = (stamp, load_vgg16_lpips_weights(path))
    return _env_loaded[0][1]


def _default_init(widths=VGG16_WIDTHS):
    sd, cin = OrderedDict(), 3
    for n, co in zip(LPIPS_CONV_INDICES, widths):  # (as many layers as there are widths: 7 for the loss, 10 for the metric)
        ref = tnn.Conv2d(cin, co, 3, padding=1)
        sd[f"features.{n}.weight"], sd[f"features.{n}.bias"] = ref.weight.detach(), ref.bias.detach()
        cin = co
    return sd


class _FrozenConv(tnn.Module):
    """Conv2d(cin, cout, 3, padding=1) + ReLU with frozen parameters (channels_last memory, as nn.Conv2d keeps its weights)."""

    def __init__(self, weight, bias):
        super().__init__()
        self.weight = tnn.Parameter(weight.detach().clone().contiguous(memory_format=torch.channels_last), requires_grad=False)
        self.bias = tnn.Parameter(bias.detach().clone(), requires_grad=False)

    def forward(self, x):
        return ops.conv2d(x, self.weight, self.bias, stride=1, pad=1, act="relu")


class _Features(tnn.Module):
    """The Sequential of the reference with only the parametrised entries registered, under torchvision's indices."""

    indices, pool_after = CONV_INDICES, POOL_AFTER

    def __init__(self, sd):
        super().__init__()
        for n in self.indices:
            self.add_module(str(n), _FrozenConv(sd[f"features.{n}.weight"], sd[f"features.{n}.bias"]))

    def forward(self, x, taps=None):
        """-> the last layer's output; with a list `taps`, the outputs (after the ReLU, before a pool) of the convolutions in
        LPIPS_TAP_AFTER are appended to it."""
        for n in self.indices:
            x = getattr(self, str(n))(x)
            if taps is not None and n in LPIPS_TAP_AFTER:
                taps.append(x)
            if n in self.pool_after:
                x = ops.max_pool2x2(x)
        return x


class LpipsFeatures(_Features):
    """The feature stack of the reference's LPIPS (utils/metrics.py:206-282): the ten convolutions up to relu4_3 with pools behind
    layers 2, 7 and 14, built from the 20-entry dict of registered_vgg16_lpips_weights().  forward(x) takes a NORMALISED NHWC tensor
    and returns the four tapped NHWC tensors relu1_2, relu2_2, relu3_3, relu4_3.  (The reference's Sequential also runs the conv5 block
    and discards its output; this one stops at the last tap.)  Frozen, always in eval mode."""

    indices, pool_after = LPIPS_CONV_INDICES, LPIPS_POOL_AFTER

    def __init__(self, sd, device=None):
        super().__init__(sd)
        if device is not None:
            self.to(device)
        super().train(False)

    def train(self, mode=True):
        return super().train(False)

    def forward(self, x):
        taps = []
        with torch.no_grad():
            super().forward(x, taps)
        return taps


class PerceptualLoss(tnn.Module):
    """mse(features(norm(pred)), features(norm(target))), the reference's PerceptualLoss.forward.  `weights`: a path or mapping for
    load_vgg16_weights; None builds the real VGG16 widths (64, 64, 128, 128, 256, 256, 256) with torch's default convolution init --
    for tests and benchmarks: that is NOT the pretrained network.  state_dict keys are the reference's features.{0,2,5,7,10,12,14}.
    {weight,bias}; every parameter is frozen and the module stays in eval mode.

    `features` is the stack itself, callable like the reference's Sequential on a NORMALISED NHWC tensor; `features_of(x)` goes from an
    image to its relu3_3 features, so a caller can compute one tensor's features once and use them in several terms (feature_mse)."""

    def __init__(self, weights=None, device=None):
        super().__init__()
        self.features = _Features(load_vgg16_weights(weights) if weights is not None else _default_init())
        self.device = device
        if device is not None:
            self.to(device)
        super().train(False)

    def train(self, mode=True):
        return super().train(False)  # frozen: the reference calls features.eval() once and never trains it

    def norm(self, *xs):
        """_norm_input of one or several same-shape images (logical NCHW, or NHWC buffers seen as NCHW), in two launches for all."""
        return ops.vgg_prep(*[ops.to_nhwc(x) for x in xs])

    def features_of(self, x):
        """The relu3_3 features (NHWC [B, H/4, W/4, C]) of an image; under no_grad when x needs no gradient."""
        if x.requires_grad and torch.is_grad_enabled():
            return self.features(self.norm(x))
        with torch.no_grad():
            return self.features(self.norm(x))

    @staticmethod
    def feature_mse(f_pred, f_target, scale=1.0):
        """scale * mse of two feature tensors; the gradient reaches f_pred only."""
        return ops.recon_loss(f_pred, f_target.detach(), "mse", scale)

    def forward(self, pred, target, scale=1.0):
        """scale * F.mse_loss(features(norm(pred)), features(norm(target))); both images are normalised in the same two launches."""
        two_sided = target.requires_grad and torch.is_grad_enabled()  # (the reference lets the gradient reach both operands)
        p, t = self.norm(pred, target)
        if two_sided:
            fp, ft = self.features(p), self.features(t)
            # d mse / d ft at (fp, ft) is d mse / d first operand at (ft, fp): the second term adds that gradient and no value
            mirrored = self.feature_mse(ft, fp, scale)
            return self.feature_mse(fp, ft, scale) + (mirrored - mirrored.detach())
        with torch.no_grad():
            ft = self.features(t)
        return self.feature_mse(self.features(p), ft, scale)

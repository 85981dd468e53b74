"""The Inception-v3 feature stack behind rFID (the reference's utils/metrics.py:360-450 InceptionV3: torchvision's inception_v3 with
`fc` replaced by the identity and transform_input=False, run from Conv2d_1a_3x3 to the global average pool) on the forward-only HIP
kernels of csrc/inception.hip (ops.infer_conv2d / infer_pool3x3 / infer_global_mean).

This build fetches no weights.  The caller registers the ones they already have -- `use_inception_weights(path, mapping or module)`,
or the environment variable MOVAE_INCEPTION_WEIGHTS=/path as the fallback -- and metrics.fid and the final evaluation's rFID then
produce numbers; with nothing registered rFID stays NaN, as the reference gives when it cannot load the network.

The accepted source is a torchvision inception_v3 state_dict: every BasicConv2d is `<name>.conv.weight` (no bias) plus
`<name>.bn.{weight, bias, running_mean, running_var}`; AuxLogits.* and *.num_batches_tracked are ignored.  `fc.weight` / `fc.bias`, the
classifier the Inception Score needs, are kept when the source has them (InceptionWeights.fc_weight / fc_bias; rFID does not use
them and a source without them loads all the same).  The eval-mode
BatchNorm (eps 1e-3) is folded at load, in float64, into a per-channel scale and shift applied in the convolution's epilogue; the
convolution weight itself stays as stored.

THE TOPOLOGY BELOW IS STATED FROM KNOWLEDGE OF torchvision's public definition; torchvision was not available where this was
written, so it has not been compared with the real module.  The strict shape check against the state_dict a user registers is the
only architecture check there is: a real inception_v3 state_dict that loads has at least the layer names, kernel sizes and channel
chaining this table expects.  Any channel widths that chain consistently are accepted (the test fixture is the topology at 1/8
width)."""
import os
from collections import OrderedDict

import torch

from . import ops

BN_EPS = 1e-3
ENV_VAR = "MOVAE_INCEPTION_WEIGHTS"
_PREFIXES = ("", "model.", "inception.")
_BN_LEAVES = ("weight", "bias", "running_mean", "running_var")

# a convolution: (kh, kw, stride, pad_h, pad_w); every layer not named here is 1x1, stride 1, no padding
_K3, _K3P, _K3S = (3, 3, 1, 0, 0), (3, 3, 1, 1, 1), (3, 3, 2, 0, 0)
_R7, _C7 = (1, 7, 1, 0, 3), (7, 1, 1, 3, 0)  # a row of seven / a column of seven
_R3, _C3 = (1, 3, 1, 0, 1), (3, 1, 1, 1, 0)
_P1 = (1, 1, 1, 0, 0)

#: the stem: a chain of layer names and "max" (3x3, stride 2, no padding)
STEM = (("Conv2d_1a_3x3", _K3S), ("Conv2d_2a_3x3", _K3), ("Conv2d_2b_3x3", _K3P), "max", ("Conv2d_3b_1x1", _P1), ("Conv2d_4a_3x3", _K3), "max")


def _block_a(name):
    return (name, (
        (("branch1x1", _P1),),
        (("branch5x5_1", _P1), ("branch5x5_2", (5, 5, 1, 2, 2))),
        (("branch3x3dbl_1", _P1), ("branch3x3dbl_2", _K3P), ("branch3x3dbl_3", _K3P)),
        ("avg", ("branch_pool", _P1))))


def _block_c(name):
    return (name, (
        (("branch1x1", _P1),),
        (("branch7x7_1", _P1), ("branch7x7_2", _R7), ("branch7x7_3", _C7)),
        (("branch7x7dbl_1", _P1), ("branch7x7dbl_2", _C7), ("branch7x7dbl_3", _R7), ("branch7x7dbl_4", _C7), ("branch7x7dbl_5", _R7)),
        ("avg", ("branch_pool", _P1))))


def _block_e(name):
    return (name, (
        (("branch1x1", _P1),),
        (("branch3x3_1", _P1), ("branch3x3_2a", _R3)),
        (("branch3x3_1", _P1), ("branch3x3_2b", _C3)),
        (("branch3x3dbl_1", _P1), ("branch3x3dbl_2", _K3P), ("branch3x3dbl_3a", _R3)),
        (("branch3x3dbl_1", _P1), ("branch3x3dbl_2", _K3P), ("branch3x3dbl_3b", _C3)),
        ("avg", ("branch_pool", _P1))))


#: the Mixed blocks: (name, paths).  A path is a chain of (layer, geometry) and "avg" / "max" steps; the block's output is the channel
#: concatenation of the paths' results in this order.  Paths that start with the same steps share them (Mixed_7b / 7c: branch3x3_1
#: feeds both _2a and _2b), and the executor computes a shared step once.
BLOCKS = (
    _block_a("Mixed_5b"), _block_a("Mixed_5c"), _block_a("Mixed_5d"),
    ("Mixed_6a", (
        (("branch3x3", _K3S),),
        (("branch3x3dbl_1", _P1), ("branch3x3dbl_2", _K3P), ("branch3x3dbl_3", _K3S)),
        ("max",))),
    _block_c("Mixed_6b"), _block_c("Mixed_6c"), _block_c("Mixed_6d"), _block_c("Mixed_6e"),
    ("Mixed_7a", (
        (("branch3x3_1", _P1), ("branch3x3_2", _K3S)),
        (("branch7x7x3_1", _P1), ("branch7x7x3_2", _R7), ("branch7x7x3_3", _C7), ("branch7x7x3_4", _K3S)),
        ("max",))),
    _block_e("Mixed_7b"), _block_e("Mixed_7c"),
)
#: the smallest input the stack accepts (Mixed_7a's stride-2 windows need 3 x 3); the metric always feeds 299 x 299
MIN_SIDE = 75


def conv_layers():
    """[(full layer name, (kh, kw, stride, pad_h, pad_w)), ...] of all 94 BasicConv2d layers, in state_dict order of first use."""
    out, seen = [], set()
    for step in STEM:
        if step not in ("max", "avg"):
            out.append(step)
    for block, paths in BLOCKS:
        for path in paths:
            for step in path:
                if step not in ("max", "avg") and (block, step[0]) not in seen:
                    seen.add((block, step[0]))
                    out.append((f"{block}.{step[0]}", step[1]))
    return out


class InceptionWeights(OrderedDict):
    """load_inception_weights' result; feature_dim: the channels of Mixed_7c's output (2048 at the real widths).  The classifier is
    carried in attributes, not items (the items are the 94 layers): fc_weight [num_classes, feature_dim] and fc_bias [num_classes]
    fp32, or None / None / 0 for a source without `fc`."""

    feature_dim = 0
    fc_weight = None
    fc_bias = None
    num_classes = 0


def _open(src):
    if isinstance(src, (str, os.PathLike)):
        src = torch.load(os.fspath(src), map_location="cpu", weights_only=True)
    if hasattr(src, "state_dict") and not hasattr(src, "keys"):
        src = src.state_dict()
    if isinstance(src, dict) and "state_dict" in src and not any(str(k).endswith(".weight") for k in src):
        src = src["state_dict"]
    return src


def _get(src, key):
    found = next((p + key for p in _PREFIXES if p + key in src), None)
    if found is None:
        raise ValueError(f"Inception-v3 weights: missing {key} (looked for {', '.join(p + key for p in _PREFIXES)})")
    return found, torch.as_tensor(src[found]).detach().to(device="cpu")


def _take_conv(src, name, geom, cin, out):
    """Validates layer `name` (cin input channels), folds its BatchNorm and stores weight / scale / shift in out; -> Cout."""
    kh, kw = geom[0], geom[1]
    found, w = _get(src, f"{name}.conv.weight")
    if w.dim() != 4 or tuple(w.shape[1:]) != (cin, kh, kw):
        raise ValueError(f"Inception-v3 weights: {found} has shape {tuple(w.shape)}, expected [Cout, {cin}, {kh}, {kw}]")
    co = w.shape[0]
    bn = {}
    for leaf in _BN_LEAVES:
        f, t = _get(src, f"{name}.bn.{leaf}")
        if tuple(t.shape) != (co,):
            raise ValueError(f"Inception-v3 weights: {f} has shape {tuple(t.shape)}, expected [{co}]")
        bn[leaf] = t.double()
    scale = bn["weight"] / torch.sqrt(bn["running_var"] + BN_EPS)
    shift = bn["bias"] - bn["running_mean"] * scale
    out[f"{name}.weight"] = w.float().contiguous()
    out[f"{name}.scale"] = scale.float()
    out[f"{name}.shift"] = shift.float()
    return co


def load_inception_weights(src):
    """-> OrderedDict {"<layer>.weight" ([Cout, Cin, kh, kw] fp32), "<layer>.scale", "<layer>.shift" ([Cout] fp32: the eval-mode
    BatchNorm, eps 1e-3, folded in float64: s = gamma / sqrt(var + eps), t = beta - mean * s, rounded to fp32 once)} for the 94
    layers of conv_layers(), from a path (read with torch.load(..., weights_only=True)), a mapping or a module.  Accepted key forms:
    `<layer>.conv.weight` / `<layer>.bn.*` bare (a torchvision inception_v3 state_dict) or under `model.` (the reference's wrapper).
    AuxLogits.* and *.num_batches_tracked are ignored; fc.weight [C, feature_dim] and fc.bias [C] go, when both are present, into the
    result's fc_weight / fc_bias / num_classes attributes (not its items).  Any channel widths that chain through the topology are
    accepted; a missing key or a wrong shape raises ValueError naming the key."""
    src = _open(src)
    out = InceptionWeights()
    c = 3
    for step in STEM:
        if step != "max":
            c = _take_conv(src, step[0], step[1], c, out)
    for block, paths in BLOCKS:
        widths, total = {}, 0  # (block-local layer chain) -> its Cout
        for path in paths:
            cp = c
            for i, step in enumerate(path):
                if step in ("max", "avg"):
                    continue
                key = path[: i + 1]
                if key not in widths:
                    widths[key] = _take_conv(src, f"{block}.{step[0]}", step[1], cp, out)
                cp = widths[key]
            total += cp
        c = total
    out.feature_dim = c
    _take_fc(src, out)
    return out


def _take_fc(src, out):
    """The classifier, when the source has one: validated against feature_dim and kept in out's attributes."""
    found = {leaf: next((p + f"fc.{leaf}" for p in _PREFIXES if p + f"fc.{leaf}" in src), None) for leaf in ("weight", "bias")}
    if found["weight"] is None and found["bias"] is None:
        return
    for leaf, key in found.items():
        if key is None:
            raise ValueError(f"Inception-v3 weights: fc.{leaf} is missing while fc.{'bias' if leaf == 'weight' else 'weight'} is present")
    w = torch.as_tensor(src[found["weight"]]).detach().to(device="cpu")
    b = torch.as_tensor(src[found["bias"]]).detach().to(device="cpu")
    if w.dim() != 2 or w.size(0) < 1 or w.size(1) != out.feature_dim:
        raise ValueError(f"Inception-v3 weights: {found['weight']} has shape {tuple(w.shape)}, expected [C, {out.feature_dim}]")
    if tuple(b.shape) != (w.size(0),):
        raise ValueError(f"Inception-v3 weights: {found['bias']} has shape {tuple(b.shape)}, expected [{w.size(0)}]")
    out.fc_weight, out.fc_bias, out.num_classes = w.float().contiguous(), b.float().contiguous(), int(w.size(0))


_registered = [None]
_env_loaded = [None]  # ((path, mtime_ns), weights): the environment fallback is read once per file


def use_inception_weights(src):
    """Register the Inception-v3 weights of this process (a path, a mapping or a module, validated and folded now by
    load_inception_weights); None removes the registration.  metrics.fid, metrics.inception_features and the final evaluation's rFID
    use them."""
    _registered[0] = None if src is None else load_inception_weights(src)


def registered_inception_weights():
    """The registered weights, else those at $MOVAE_INCEPTION_WEIGHTS, else None.  The same object is returned until the registration
    (or the file behind the environment variable) changes: metrics keys its cached extractor on it."""
    if _registered[0] is not None:
        return _registered[0]
    path = os.environ.get("MOVAE_INCEPTION_WEIGHTS")  # (ENV_VAR; spelled out: INTEGRATION.md's switch table is checked against the source)
    if not path:
        return None
    stamp = (path, os.stat(path).st_mtime_ns)
    if _env_loaded[0] is None or _env_loaded[0][0] != stamp:
        _env_loaded[0] = (stamp, load_inception_weights(path))
    return _env_loaded[0][1]


def real_widths():
    """{full layer name: Cout} of torchvision's inception_v3 (stated from knowledge, like the topology)."""
    out = {"Conv2d_1a_3x3": 32, "Conv2d_2a_3x3": 32, "Conv2d_2b_3x3": 64, "Conv2d_3b_1x1": 80, "Conv2d_4a_3x3": 192}
    for block, pool in (("Mixed_5b", 32), ("Mixed_5c", 64), ("Mixed_5d", 64)):
        out.update({f"{block}.{k}": v for k, v in (("branch1x1", 64), ("branch5x5_1", 48), ("branch5x5_2", 64), ("branch3x3dbl_1", 64),
                                                   ("branch3x3dbl_2", 96), ("branch3x3dbl_3", 96), ("branch_pool", pool))})
    out.update({f"Mixed_6a.{k}": v for k, v in (("branch3x3", 384), ("branch3x3dbl_1", 64), ("branch3x3dbl_2", 96), ("branch3x3dbl_3", 96))})
    for block, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        out.update({f"{block}.{k}": v for k, v in (("branch1x1", 192), ("branch7x7_1", c7), ("branch7x7_2", c7), ("branch7x7_3", 192),
                                                   ("branch7x7dbl_1", c7), ("branch7x7dbl_2", c7), ("branch7x7dbl_3", c7),
                                                   ("branch7x7dbl_4", c7), ("branch7x7dbl_5", 192), ("branch_pool", 192))})
    out.update({f"Mixed_7a.{k}": v for k, v in (("branch3x3_1", 192), ("branch3x3_2", 320), ("branch7x7x3_1", 192), ("branch7x7x3_2", 192),
                                                ("branch7x7x3_3", 192), ("branch7x7x3_4", 192))})
    for block in ("Mixed_7b", "Mixed_7c"):
        out.update({f"{block}.{k}": v for k, v in (("branch1x1", 320), ("branch3x3_1", 384), ("branch3x3_2a", 384), ("branch3x3_2b", 384),
                                                   ("branch3x3dbl_1", 448), ("branch3x3dbl_2", 384), ("branch3x3dbl_3a", 384),
                                                   ("branch3x3dbl_3b", 384), ("branch_pool", 192))})
    return out


def random_state_dict(seed=0, div=1):
    """A state_dict in torchvision's layout at the real widths / div with seeded He-normal weights and non-trivial BatchNorm
    statistics -- for benchmarks and tests: that is NOT the pretrained network."""
    g = torch.Generator().manual_seed(int(seed))
    widths = {k: v // div for k, v in real_widths().items()}
    sd = OrderedDict()

    def add(name, geom, cin):
        co = widths[name]
        kh, kw = geom[0], geom[1]
        sd[f"{name}.conv.weight"] = torch.randn((co, cin, kh, kw), generator=g) * (2.0 / (cin * kh * kw)) ** 0.5
        sd[f"{name}.bn.weight"] = torch.rand(co, generator=g) * 0.6 + 0.7
        sd[f"{name}.bn.bias"] = torch.rand(co, generator=g) * 0.5 - 0.2
        sd[f"{name}.bn.running_mean"] = torch.randn(co, generator=g) * 0.2
        sd[f"{name}.bn.running_var"] = torch.rand(co, generator=g) * 0.8 + 0.6
        return co

    c = 3
    for step in STEM:
        if step != "max":
            c = add(step[0], step[1], c)
    for block, paths in BLOCKS:
        total, seen = 0, {}
        for path in paths:
            cp = c
            for i, step in enumerate(path):
                if step in ("max", "avg"):
                    continue
                if path[: i + 1] not in seen:
                    seen[path[: i + 1]] = add(f"{block}.{step[0]}", step[1], cp)
                cp = seen[path[: i + 1]]
            total += cp
        c = total
    return sd


class InceptionFeatures:
    """The stack on one device: forward(x) takes a NORMALISED NHWC [n, h, w, 3] fp32 tensor (h, w >= 75; ops.inception_prep's output is
    299 x 299) and returns the [n, D] pooled features (D = 2048 at the real widths).  Every branch of a block writes its slice of the
    block's concat buffer; intermediate and concat buffers are allocated once per input shape and reused (the last two shapes are kept).
    Frozen; no autograd."""

    def __init__(self, weights, device):
        self.device = torch.device(device)
        self.feature_dim = weights.feature_dim
        self.layers = {}
        for name, _ in conv_layers():
            w = weights[f"{name}.weight"].permute(0, 2, 3, 1).contiguous().to(self.device)  # [Co][KH][KW][Ci]
            self.layers[name] = (w, weights[f"{name}.scale"].to(self.device), weights[f"{name}.shift"].to(self.device))
        self.num_classes = weights.num_classes
        self.fc = None if not weights.num_classes else (weights.fc_weight.to(self.device), weights.fc_bias.to(self.device))
        self._cache, self._bufs = OrderedDict(), {}  # input shape -> its buffers (the two most recent: a full and a partial chunk)

    def _select(self, shape):
        self._bufs = self._cache.setdefault(shape, {})
        self._cache.move_to_end(shape)
        while len(self._cache) > 2:
            self._cache.popitem(last=False)

    def release(self):
        """Drops the cached buffers (the weights stay)."""
        self._cache, self._bufs = OrderedDict(), {}

    def features_of(self, images):
        """NCHW [n, 3, h, w] images (h, w <= 299) -> their [n, D] features: ops.inception_prep into a cached buffer, then forward.
        The result is a cached buffer too: copy it before the next call."""
        shape = (images.size(0), ops.INCEPTION_SIDE, ops.INCEPTION_SIDE, 3)
        self._select(shape)
        return self.forward(ops.inception_prep(images, self._buf("prep", shape)))

    @property
    def has_classifier(self):
        return self.fc is not None

    def probs_of(self, images):
        """NCHW [n, 3, h, w] images (h, w <= 299) -> their [n, C] class probabilities, calculate_inception_score's pass
        (utils/metrics.py:872-889): the BILINEAR input pipeline, the stack, the classifier (eval-mode dropout is the identity) and the
        softmax.  A cached buffer, like features_of's result."""
        if self.fc is None:
            raise RuntimeError("the registered Inception-v3 weights have no classifier (fc.weight / fc.bias): the Inception Score "
                               "cannot be computed from them")
        shape = (images.size(0), ops.INCEPTION_SIDE, ops.INCEPTION_SIDE, 3)
        self._select(shape)
        feats = self.forward(ops.inception_prep(images, self._buf("prep", shape), filter="bilinear"))
        return ops.linear_softmax(feats, self.fc[0], self.fc[1], self._buf("probs", (images.size(0), self.num_classes)))

    def _buf(self, key, shape):
        t = self._bufs.get(key)
        if t is None or tuple(t.shape) != tuple(shape):
            t = torch.empty(shape, dtype=torch.float32, device=self.device)
            self._bufs[key] = t
        return t

    def _conv(self, x, name, geom, out, offset):
        w, scale, shift = self.layers[name]
        kh, kw, stride, ph, pw = geom
        n, h, wd, _ = x.shape
        if out is None:
            out = self._buf(name, (n, ops.conv_out_size(h, kh, stride, ph), ops.conv_out_size(wd, kw, stride, pw), w.size(0)))
        return ops.infer_conv2d(x, w, scale, shift, stride, (ph, pw), out, offset)

    def _pool(self, x, mode, key, out, offset):
        n, h, wd, c = x.shape
        if out is None:
            shape = (n, (h - 3) // 2 + 1, (wd - 3) // 2 + 1, c) if mode == "max" else (n, h, wd, c)
            out = self._buf(key, shape)
        return ops.infer_pool3x3(x, mode, out, offset)

    @torch.no_grad()
    def forward(self, x):
        if x.dim() != 4 or x.size(3) != 3 or min(x.shape[1:3]) < MIN_SIDE:
            raise ValueError(f"InceptionFeatures takes NHWC [n, h, w, 3] with h, w >= {MIN_SIDE}, got {tuple(x.shape)}")
        self._select(tuple(x.shape))
        for i, step in enumerate(STEM):
            x = self._pool(x, "max", f"stem.max{i}", None, 0) if step == "max" else self._conv(x, step[0], step[1], None, 0)
        for block, paths in BLOCKS:
            x = self._block(x, block, paths)
        return ops.infer_global_mean(x, self._buf("features", (x.size(0), x.size(3))))

    __call__ = forward

    def _path_width(self, block, path, cin):
        last = path[-1]
        if last in ("max", "avg"):
            return cin if len(path) == 1 else self.layers[f"{block}.{path[-2][0]}"][0].size(0)
        return self.layers[f"{block}.{last[0]}"][0].size(0)

    def _block(self, x, block, paths):
        n, h, wd, cin = x.shape
        widths = [self._path_width(block, p, cin) for p in paths]
        # the block's spatial size: that of its first path's last step (every path agrees)
        ho, wo = h, wd
        for step in paths[0]:
            if step == "max":
                ho, wo = (ho - 3) // 2 + 1, (wo - 3) // 2 + 1
            elif step != "avg":
                kh, kw, s, ph, pw = step[1]
                ho, wo = ops.conv_out_size(ho, kh, s, ph), ops.conv_out_size(wo, kw, s, pw)
        out = self._buf(block, (n, ho, wo, sum(widths)))
        done, at = {}, 0
        for path, width in zip(paths, widths):
            cur = x
            for i, step in enumerate(path):
                key, last = path[: i + 1], i == len(path) - 1
                if not last and key in done:
                    cur = done[key]
                    continue
                dst, off = (out, at) if last else (None, 0)
                if step in ("max", "avg"):
                    cur = self._pool(cur, step, f"{block}.{step}", dst, off)
                else:
                    cur = self._conv(cur, f"{block}.{step[0]}", step[1], dst, off)
                if not last:
                    done[key] = cur
            at += width
        return out

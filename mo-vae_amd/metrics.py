"""Reconstruction metrics and the hypervolume of the objective vector (reference utils/metrics.py:14-203, main.py:335-463,
:659-692) on the HIP path.

`ssim` / `psnr` / `ssnr` keep the reference's signatures, return types and empty-input rules; each call is one chunk: its
[-1, 1] -> [0, 1] decision is taken over the whole input, as the reference's functions take it.  The arithmetic is one
C-ABI call (include/movae.h: movae_recon_metrics, three launches, no host read): the min-reduction that decides the
normalisation, the fused SSIM / MSE / signal-variance pass, and a fixed-order finalize.

`lpips` is the reference's utils/metrics.py:290-357 on VGG16 weights the caller registered (perceptual.use_vgg16_weights): the
input normalisation and the feature stack of the perceptual loss, extended to relu4_3 (perceptual.LpipsFeatures), then one
movae_lpips_layer per tapped layer and one movae_lpips_finalize (csrc/lpips.hip); `lpips_into` is the form without a host read.

`fid` is the reference's calculate_fid (utils/metrics.py:513-615) on Inception-v3 weights the caller registered
(inception.use_inception_weights): `inception_features` runs the input pipeline and the feature stack on the forward-only kernels of
csrc/inception.hip, `fid_from_features` is the Frechet distance of the two feature sets in float64.

`ReconMetricAccumulator` is the collection of main.py:376-463 without the host copies: (real, recon) pairs are taken batch by
batch up to `max_samples`, cut into the reference's 128-sample chunks (the chunks of the concatenated collection, so they
straddle loader batches), and each chunk is scored on the device as soon as it is complete.  `result()` is the one host read.

`build_hv_indicator` gives pymoo's HV for the single point the reference passes it, in closed form (pymoo is not needed).
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L

CHUNK = 128  # main.py:335 batch_size_metric
NAN_RESULT = {"rfid": float("nan"), "psnr": float("nan"), "ssim": float("nan"), "lpips": float("nan")}


def _check_window(window_size):
    if not isinstance(window_size, (int, np.integer)) or window_size < 3 or window_size > 15 or window_size % 2 == 0:
        raise ValueError(f"window_size must be an odd integer in 3..15, got {window_size!r}")


def _operand(t):
    L.require_gpu(t)
    if t.dim() != 4:
        raise ValueError(f"expected (B, C, H, W) images, got shape {tuple(t.shape)}")
    return t if t.dtype == torch.float32 else t.float()


def _workspace(device, nbytes):
    ws = L.workspace(device)
    if ws.numel() >= nbytes:
        return ws
    return torch.zeros(nbytes, dtype=torch.uint8, device=device)  # (the counter header must start at zero)


def recon_metrics_into(out, real, recon, window_size=11, max_val=1.0):
    """One chunk through movae_recon_metrics: out (device float32[3 + 3 n]) receives [ssim, psnr, ssnr, per-image ssim (n),
    per-image mse (n), per-image ssnr (n)].  Both operands are read through their strides (no copy)."""
    _check_window(window_size)
    real, recon = _operand(real), _operand(recon)
    if real.shape != recon.shape:
        raise ValueError(f"image shapes differ: {tuple(real.shape)} vs {tuple(recon.shape)}")
    if real.device != recon.device:
        raise ValueError("real and recon must be on the same device")
    n, c, h, w = real.shape
    if out.numel() < 3 + 3 * n or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 tensor of 3 + 3 n elements")
    lib = L.load()
    nbytes = lib.movae_recon_metrics_ws_bytes(n, c, h, w)
    ws = _workspace(real.device, nbytes)
    L.call("movae_recon_metrics", real.data_ptr(), *real.stride(), recon.data_ptr(), *recon.stride(), n, c, h, w, int(window_size),
           float(max_val), out.data_ptr(), ws.data_ptr(), ws.numel(), L.stream_ptr(real.device))
    return out


def _run(img1, img2, window_size=11, max_val=1.0):
    out = torch.empty(3 + 3 * img1.size(0), dtype=torch.float32, device=img1.device)
    return recon_metrics_into(out, img1, img2, window_size, max_val)


def ssim(img1, img2, window_size=11, size_average=True):
    """utils/metrics.py:14-80: mean SSIM (0-d tensor) or per-image SSIM ((B,) tensor) on the device."""
    if img1.numel() == 0 or img2.numel() == 0:
        device = img1.device if img1.numel() > 0 else img2.device
        dtype = img1.dtype if img1.numel() > 0 else img2.dtype
        if size_average:
            return torch.tensor(float("nan"), device=device, dtype=dtype)
        b = img1.size(0) if img1.numel() > 0 else (img2.size(0) if img2.numel() > 0 else 0)
        if b == 0:
            return torch.tensor([], device=device, dtype=dtype)
        return torch.full((b,), float("nan"), device=device, dtype=dtype)
    _check_window(window_size)
    out = _run(img1, img2, window_size)
    n = img1.size(0)
    return out[0] if size_average else out[3: 3 + n]


def psnr(img1, img2, max_val=1.0):
    """utils/metrics.py:157-203: mean over the images of 20 log10(max_val) - 10 log10(max(mse, 1e-10)) (Python float)."""
    if img1.numel() == 0 or img2.numel() == 0:
        return float("nan")
    return float(_run(img1, img2, max_val=max_val)[1].item())


def ssnr(img1, img2):
    """utils/metrics.py:108-154: mean over the images of 10 log10(var(img1) / mse), both clamped at 1e-10 (Python float)."""
    if img1.numel() == 0 or img2.numel() == 0:
        return float("nan")
    return float(_run(img1, img2)[2].item())


# ---- LPIPS ----------------------------------------------------------------------------------------------------------------
LPIPS_MIN_SIDE = 8    # three 2x2 pools in front of conv4: the third needs a 2x2 input
LPIPS_MIN_WIDTH = 32  # main.py:335 min_size_for_lpips, the final evaluation's gate on size(-1)
_lpips_features = {}  # device -> (the registered 20-entry dict, the LpipsFeatures built from it)


def _lpips_weights():
    from . import perceptual

    return perceptual.registered_vgg16_lpips_weights()


def _features_on(device, weights):
    """The feature extractor of this device, built once per registration (a new registration is a new dict object)."""
    from . import perceptual

    key = (device.type, device.index)
    hit = _lpips_features.get(key)
    if hit is None or hit[0] is not weights:
        hit = (weights, perceptual.LpipsFeatures(weights, device=device))
        _lpips_features[key] = hit
    return hit[1]


def _lpips_operand(t):
    from . import ops

    t = _operand(t)
    if t.size(1) == 1:
        t = t.expand(-1, 3, -1, -1)  # utils/metrics.py:271-272
    if t.size(1) != 3:
        raise ValueError(f"lpips takes images of 1 or 3 channels, got shape {tuple(t.shape)}")
    return ops.to_nhwc(t).contiguous()


def feature_distance_into(out, pairs):
    """The distance part alone: `pairs` is a list (one entry per layer, at most 8) of two contiguous fp32 NHWC feature tensors
    [n, h, w, c] with c % 4 == 0.  out (device float32[1 + n]) receives the mean over the layers of the pixel-averaged squared
    distance between the channel-normalised features, as [mean over the images, per-image values]: one movae_lpips_layer per
    pair and one movae_lpips_finalize, no host read."""
    first = pairs[0][0]
    L.require_gpu(first)
    n, dev = first.size(0), first.device
    for f1, f2 in pairs:
        if not (f1.dim() == 4 and f1.shape == f2.shape and f1.size(0) == n and f1.dtype == f2.dtype == torch.float32
                and f1.is_contiguous() and f2.is_contiguous() and f1.device == f2.device == dev):
            raise ValueError(f"feature pairs must be contiguous float32 NHWC tensors of one shape and batch, got {tuple(f1.shape)} / "
                             f"{tuple(f2.shape)}")
    if out.numel() < 1 + n or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError("out must be a contiguous float32 tensor of 1 + n elements on the features' device")
    lib = L.load()
    st = L.stream_ptr(dev)
    # the partials of all layers, one region each, behind the workspace's header
    sizes = [lib.movae_lpips_ws_bytes(*f.shape) for f, _ in pairs]
    ws = _workspace(dev, L.WS_HEADER_BYTES + sum(sizes))
    parts, at = [], ws.data_ptr() + L.WS_HEADER_BYTES
    for (f1, f2), nbytes in zip(pairs, sizes):
        L.call("movae_lpips_layer", f1.data_ptr(), f2.data_ptr(), *f1.shape, 1.0, at, nbytes, st)
        parts.append(at)
        at += nbytes
    k = len(pairs)
    ints = C.c_int * k
    L.call("movae_lpips_finalize", k, (C.c_void_p * k)(*parts), *[ints(*[f.shape[d] for f, _ in pairs]) for d in (1, 2, 3)], n,
           out.data_ptr(), st)
    return out


@torch.no_grad()
def lpips_into(out, real, recon):
    """One chunk of the reference's lpips (utils/metrics.py:290-357) on the device, without a host read: out (device
    float32[1 + n]) receives [mean over the images, per-image values].  Both operands are normalised by vgg_prep's two launches
    (each one's [-1, 1] decision over the whole operand) straight into the two halves of one [2 n, H, W, 3] buffer, the feature
    stack runs once on the 2 n images, then one movae_lpips_layer per tap on the two halves of its features and one
    movae_lpips_finalize."""
    weights = _lpips_weights()
    if weights is None:
        raise RuntimeError("lpips needs VGG16 weights with the conv4 block (features.17 / 19 / 21): register them with "
                           "perceptual.use_vgg16_weights(path or state_dict); nothing is downloaded")
    if real.shape != recon.shape:
        raise ValueError(f"image shapes differ: {tuple(real.shape)} vs {tuple(recon.shape)}")
    if real.device != recon.device:
        raise ValueError("real and recon must be on the same device")
    if real.dim() == 4 and min(real.shape[2:]) < LPIPS_MIN_SIDE:
        raise ValueError(f"lpips needs images of at least {LPIPS_MIN_SIDE} x {LPIPS_MIN_SIDE} (three 2x2 pools in front of conv4), "
                         f"got {tuple(real.shape)}")
    a, b = _lpips_operand(real), _lpips_operand(recon)
    n, h, w, _ = a.shape
    dev = a.device
    lib = L.load()
    st = L.stream_ptr(dev)
    both = torch.empty((2 * n, h, w, 3), dtype=torch.float32, device=dev)
    flags = torch.empty(2, dtype=torch.int32, device=dev)
    ws = _workspace(dev, lib.movae_vgg_prep_ws_bytes(2))
    ptrs = C.c_void_p * 2
    L.call("movae_vgg_prep_fwd", 2, ptrs(a.data_ptr(), b.data_ptr()), ptrs(both[:n].data_ptr(), both[n:].data_ptr()), flags.data_ptr(),
           a.numel(), ws.data_ptr(), ws.numel(), st)
    taps = _features_on(dev, weights)(both)
    return feature_distance_into(out, [(f[:n], f[n:]) for f in taps])


def lpips(img1, img2, device=None, net='vgg'):
    """utils/metrics.py:290-357: the mean over the images of the mean over relu1_2, relu2_2, relu3_3, relu4_3 of the squared distance
    between the channel-normalised VGG16 features, averaged over the pixels (Python float; NaN for an empty operand).  The weights
    are the ones registered with perceptual.use_vgg16_weights (a torchvision vgg16 state_dict serves both the loss and this metric);
    `device` moves the operands there first."""
    if net != 'vgg':
        raise ValueError(f"Network {net} not supported. Currently only 'vgg' is supported.")
    if img1.numel() == 0 or img2.numel() == 0:
        return float("nan")
    if device is not None:
        img1, img2 = img1.to(device), img2.to(device)
    out = torch.empty(1 + img1.size(0), dtype=torch.float32, device=img1.device)
    return float(lpips_into(out, img1, img2)[0].item())


# ---- FID ------------------------------------------------------------------------------------------------------------------
_inception_features = {}  # device -> (the registered weights, the InceptionFeatures built from them)


def _inception_weights():
    from . import inception

    return inception.registered_inception_weights()


def _inception_on(device, weights):
    """The Inception extractor of this device, built once per registration (a new registration is a new object)."""
    from . import inception

    key = (device.type, device.index)
    hit = _inception_features.get(key)
    if hit is None or hit[0] is not weights:
        hit = (weights, inception.InceptionFeatures(weights, device))
        _inception_features[key] = hit
    return hit[1]


def release_inception_buffers(device=None):
    """Drops the extractor's cached activation buffers (several GB for a 128-image chunk at the real widths) of one device or of
    all; the weights stay, and the next call allocates the buffers again.  The final evaluation calls it when it is done."""
    want = None if device is None else torch.device(device)
    for (kind, index), (_, net) in _inception_features.items():
        if want is None or (kind == want.type and want.index in (None, index)):
            net.release()


@torch.no_grad()
def inception_features_into(out, images, chunk=CHUNK):
    """The pooled Inception-v3 features of `images` ([N, 3, h, w] on the device, any float dtype, h, w <= 299) into out
    ([N, D] fp32 on the same device), `chunk` images at a time: calculate_fid's input pipeline in one launch (ops.inception_prep:
    the unconditional 0.5 x + 0.5 and clamp, the antialiased bicubic resize to 299 with the centre crop, the ImageNet
    normalisation), then the stack (inception.InceptionFeatures).  No host read.  A side above 299 raises NotImplementedError."""
    weights = _inception_weights()
    if weights is None:
        raise RuntimeError("FID needs Inception-v3 weights: register them with inception.use_inception_weights(path, state_dict or "
                           "module); nothing is downloaded")
    images = _operand(images)
    if images.size(1) != 3:
        raise ValueError(f"the Inception features take 3-channel images, got shape {tuple(images.shape)}")
    n = images.size(0)
    net = _inception_on(images.device, weights)
    if tuple(out.shape) != (n, net.feature_dim) or out.dtype != torch.float32 or out.device != images.device:
        raise ValueError(f"out must be a float32 [{n}, {net.feature_dim}] tensor on the images' device")
    for lo in range(0, n, int(chunk)):
        part = images[lo: lo + int(chunk)]
        out[lo: lo + part.size(0)].copy_(net.features_of(part))
    return out


def inception_features(images, chunk=CHUNK):
    """-> [N, D] fp32 on the device (D = 2048 at the real widths): extract_inception_features of utils/metrics.py:618-653 without
    the host copy."""
    from . import inception

    weights = _inception_weights()
    dim = weights.feature_dim if weights is not None else inception.InceptionWeights.feature_dim
    out = torch.empty((images.size(0), dim), dtype=torch.float32, device=images.device)
    return inception_features_into(out, images, chunk) if images.size(0) else out


def _sqrt_psd(m):
    lam, vec = torch.linalg.eigh(m)
    return (vec * lam.clamp_min(0).sqrt()) @ vec.T


def fid_from_features(real, fake):
    """utils/metrics.py:656-679 fid_from_features: |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2), means and covariances
    (divisor N - 1, np.cov's) in float64.  The trace term is the sum of the square roots of the eigenvalues of the symmetric
    S1^(1/2) S2 S1^(1/2) -- the same spectrum as S1 S2 -- from two torch.linalg.eigh calls in float64 on the host, negative
    eigenvalues (rounding of a singular covariance) clamped to 0; no scipy.  Accepts tensors (any device) or arrays [N, D]."""
    f = [torch.as_tensor(t).detach().to(dtype=torch.float64) for t in (real, fake)]
    if f[0].numel() == 0 or f[1].numel() == 0:
        return float("nan")
    mu, cov = [], []
    for t in f:
        m = t.mean(dim=0)
        d = t - m
        mu.append(m.cpu())
        cov.append(((d.T @ d) / (t.size(0) - 1)).cpu())
    diff = mu[0] - mu[1]
    root = _sqrt_psd(cov[0])
    inner = root @ cov[1] @ root
    lam = torch.linalg.eigvalsh((inner + inner.T) * 0.5)
    tr = lam.clamp_min(0).sqrt().sum()
    return float(diff.dot(diff) + torch.trace(cov[0]) + torch.trace(cov[1]) - 2.0 * tr)


def fid(real, fake, chunk=CHUNK):
    """utils/metrics.py:513-615 calculate_fid on the registered Inception-v3 weights: NaN for an empty operand, else
    fid_from_features of the two sets' inception_features."""
    if real.numel() == 0 or fake.numel() == 0:
        return float("nan")
    return fid_from_features(inception_features(real, chunk), inception_features(fake, chunk))


# ---- the generative evaluation: Inception Score, KID, precision / recall (gFID is fid_from_features) ---------------------------------
def _device_matrix(t):
    """A feature or probability set as the kernels take it: contiguous fp32 [N, D] on its device."""
    t = torch.as_tensor(t)
    L.require_gpu(t)
    return t.detach().to(dtype=torch.float32).contiguous()


@torch.no_grad()
def inception_probs(images, chunk=CHUNK):
    """-> [N, C] fp32 on the device: the class probabilities of calculate_inception_score's pass (utils/metrics.py:861-890) --
    the unconditional 0.5 x + 0.5 and clamp, the antialiased BILINEAR resize to 299 (TF.resize's default filter, not rFID's
    bicubic), centre crop, ImageNet normalisation, the stack, `fc` and the softmax -- `chunk` images at a time, without a host
    read.  Needs registered weights that carry the classifier."""
    weights = _inception_weights()
    if weights is None or not weights.num_classes:
        raise RuntimeError("the Inception Score needs Inception-v3 weights with the classifier (fc.weight, fc.bias): register them with "
                           "inception.use_inception_weights(path, state_dict or module); nothing is downloaded")
    images = _operand(images)
    if images.size(1) != 3:
        raise ValueError(f"the Inception classifier takes 3-channel images, got shape {tuple(images.shape)}")
    n = images.size(0)
    out = torch.empty((n, weights.num_classes), dtype=torch.float32, device=images.device)
    net = _inception_on(images.device, weights)
    for lo in range(0, n, int(chunk)):
        part = images[lo: lo + int(chunk)]
        out[lo: lo + part.size(0)].copy_(net.probs_of(part))
    return out


def inception_score_from_probs(probs, splits=10):
    """utils/metrics.py:895-914 on [N, C] probabilities on the device -> (mean, std) over the splits (np.std: the population
    form).  Every split's score comes from one launch (ops.inception_score_splits, fp64); (nan, nan) for an empty set and for
    N < splits, where every split of the reference is empty."""
    probs = torch.as_tensor(probs)
    if probs.dim() != 2 or probs.numel() == 0 or probs.size(0) // int(splits) < 1:
        return float("nan"), float("nan")
    from . import ops

    scores = ops.inception_score_splits(_device_matrix(probs), splits).cpu().numpy()
    return float(np.mean(scores)), float(np.std(scores))


def inception_score(images, splits=10, chunk=CHUNK):
    """utils/metrics.py:835-914 calculate_inception_score on the registered weights -> (mean, std); (nan, nan) for empty input,
    for N < splits and when no classifier weights are registered."""
    weights = _inception_weights()
    if images.numel() == 0 or images.size(0) // int(splits) < 1 or weights is None or not weights.num_classes:
        return float("nan"), float("nan")
    return inception_score_from_probs(inception_probs(images, chunk), splits)


def kid_subset_indices(n_real, n_fake, subset_size, n_subsets, seed=None):
    """The subsets of utils/metrics.py:695-699 from np.random.default_rng(seed), in the reference's order: per subset,
    choice(n_real, m, replace=False) then choice(n_fake, m, replace=False).  -> (idx_real, idx_fake), int64 [n_subsets, m]."""
    rng = np.random.default_rng(seed)
    idx_real = np.empty((n_subsets, subset_size), dtype=np.int64)
    idx_fake = np.empty((n_subsets, subset_size), dtype=np.int64)
    for s in range(n_subsets):
        idx_real[s] = rng.choice(n_real, size=subset_size, replace=False)
        idx_fake[s] = rng.choice(n_fake, size=subset_size, replace=False)
    return idx_real, idx_fake


def kid_from_features(real, fake, subset_size=50, n_subsets=50, degree=3, gamma=None, seed=None, subsets=None):
    """utils/metrics.py:682-709 kid_from_features on [N, D] feature sets on the device: the mean over the subsets of the clamped
    unbiased MMD^2 under (gamma x.y + 1)^degree, gamma = 1 / D by default, every subset in one launch (ops.kid_subsets, fp64).
    The subsets are drawn on the host (kid_subset_indices; the reference seeds nothing, `seed` makes the draw repeatable) or given
    as subsets=(idx_real, idx_fake), [S, m] each.  NaN for an empty set or m = min(subset_size, n_real, n_fake) < 2."""
    if len(real) == 0 or len(fake) == 0:
        return float("nan")
    n_real, dim = real.shape
    n_fake = fake.shape[0]
    m = min(int(subset_size), n_real, n_fake)
    if subsets is not None:
        idx_real, idx_fake = (np.asarray(torch.as_tensor(t).cpu()) for t in subsets)
        if idx_real.ndim != 2 or idx_real.shape != idx_fake.shape:
            raise ValueError(f"subsets must be two [S, m] index arrays, got {idx_real.shape} and {idx_fake.shape}")
        m = idx_real.shape[1]
    if m < 2:
        return float("nan")
    if subsets is None:
        idx_real, idx_fake = kid_subset_indices(n_real, n_fake, m, int(n_subsets), seed)
    if idx_real.shape[0] == 0:
        return float("nan")  # (np.mean of no values)
    for idx, n, what in ((idx_real, n_real, "real"), (idx_fake, n_fake, "fake")):
        if idx.min() < 0 or idx.max() >= n:
            raise ValueError(f"a subset index of the {what} set lies outside 0 .. {n - 1}")
    real, fake = _device_matrix(real), _device_matrix(fake)
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(real.device)  # noqa: E731
    from . import ops

    vals = ops.kid_subsets(real, fake, to_dev(idx_real), to_dev(idx_fake), 1.0 / dim if gamma is None else float(gamma), degree)
    return float(vals.mean().item())


def precision_recall_from_features(real, fake, k=3):
    """utils/metrics.py:712-736 precision_recall_from_features on [N, D] feature sets on the device -> (precision, recall): a
    generated sample counts when its distance to the nearest real sample is at most that real sample's k-th neighbour radius among
    the real set, and the other way round.  Four ops.knn_rows calls (R/R and F/F with k, diagonal excluded; F->R and R->F with
    k = 1) instead of four N x N cdist matrices; the comparison stays on the device.  (nan, nan) for an empty set or len <= k."""
    if len(real) == 0 or len(fake) == 0 or len(real) <= k or len(fake) <= k:
        return float("nan"), float("nan")
    from . import ops

    real, fake = _device_matrix(real), _device_matrix(fake)
    radius_real = ops.knn_rows(real, real, k, exclude_diag=True)[0][:, k - 1].clamp_min(0).sqrt()
    radius_fake = ops.knn_rows(fake, fake, k, exclude_diag=True)[0][:, k - 1].clamp_min(0).sqrt()
    d_fr, i_fr = ops.knn_rows(fake, real, 1)
    d_rf, i_rf = ops.knn_rows(real, fake, 1)
    precision = (d_fr[:, 0].clamp_min(0).sqrt() <= radius_real[i_fr.long()]).float().mean()
    recall = (d_rf[:, 0].clamp_min(0).sqrt() <= radius_fake[i_rf.long()]).float().mean()
    return float(precision.item()), float(recall.item())


# ---- collection in the reference's chunks ------------------------------------------------------------------------------
class ChunkPlanner:
    """Host-side bookkeeping of main.py:376-463 + :335-373: which samples of each loader batch are taken (the `take` cut at
    max_samples) and which chunk of the concatenated collection each of them lands in."""

    def __init__(self, max_samples, chunk=CHUNK):
        if chunk <= 0:
            raise ValueError("chunk must be positive")
        self.max_samples, self.chunk, self.seen = int(max_samples), int(chunk), 0

    @property
    def full(self):
        return self.seen >= self.max_samples

    def add(self, batch):
        """-> (take, [(chunk index, batch lo, batch hi, position in chunk), ...]) for a batch of `batch` samples."""
        take = min(int(batch), max(0, self.max_samples - self.seen))
        segs, lo = [], 0
        while lo < take:
            g = self.seen + lo
            k, pos = divmod(g, self.chunk)
            hi = min(take, lo + self.chunk - pos)
            segs.append((k, lo, hi, pos))
            lo = hi
        self.seen += take
        return take, segs


def plan_chunks(batch_sizes, max_samples, chunk=CHUNK):
    """ChunkPlanner over a whole sequence of batch sizes: -> list of (take, segments) per batch."""
    p = ChunkPlanner(max_samples, chunk)
    return [p.add(b) for b in batch_sizes]


class ReconMetricAccumulator:
    """(real, recon) batches -> the reference's rFID / PSNR / SSIM / LPIPS dict.  rFID needs a pretrained Inception: with weights
    registered (inception.use_inception_weights) the [N, D] features of real and recon are extracted chunk by chunk and kept on the
    device (2 x 10 000 x 2048 fp32 = 164 MB), and result() gives fid_from_features of the two sets under the reference's conditions
    (main.py:368: width >= min_size_for_lpips, n >= 2; 3 channels -- its TF.normalize raises on 1-channel images and the except
    leaves NaN); with nothing registered it is NaN, as the reference gives when it cannot load the network, and the Inception path
    allocates nothing.  LPIPS is scored per chunk (lpips_into) when VGG16 weights with the conv4 block are
    registered (perceptual.use_vgg16_weights) and the images are at least 32 wide, the reference's min_size_for_lpips; else NaN.
    At most one chunk is staged on the device (a chunk that lies inside one batch is scored straight from the batch's
    tensors); every chunk is scored when it completes and its ssim / psnr / lpips stay on the device until result()."""

    def __init__(self, device, max_samples, chunk=CHUNK, window_size=11):
        _check_window(window_size)
        self.device = torch.device(device)
        self.planner = ChunkPlanner(max_samples, chunk)
        self.chunk, self.window_size = int(chunk), window_size
        self._stage = None  # (real, recon) NCHW float32 [chunk, C, H, W]
        self._fill = 0
        self._outs = []
        self._lpips = None
        self._fid = None   # decided at the first chunk, like _lpips
        self._feats = ([], [])  # per chunk: the [n, D] features of real / recon

    @property
    def full(self):
        return self.planner.full

    @property
    def count(self):
        return self.planner.seen

    def _score(self, real, recon):
        vals = _run(real, recon, self.window_size)[:2]
        if self._lpips is None:  # decided once, at the first chunk: main.py:344, :357 gate on the width alone
            self._lpips = (_lpips_weights() is not None and real.size(-1) >= LPIPS_MIN_WIDTH and real.size(-2) >= LPIPS_MIN_SIDE
                           and real.size(1) in (1, 3))
        if self._lpips:
            lp = lpips_into(torch.empty(1 + real.size(0), dtype=torch.float32, device=real.device), real, recon)
            vals = torch.cat([vals, lp[:1]])
        self._outs.append(vals)
        if self._fid is None:
            self._fid = _inception_weights() is not None and real.size(-1) >= LPIPS_MIN_WIDTH and real.size(1) == 3
        if self._fid:
            try:
                for keep, images in zip(self._feats, (real, recon)):
                    keep.append(inception_features(images, self.chunk))
            except NotImplementedError as e:  # (a side above 299: main.py:371-372 prints a warning and leaves NaN)
                print(f"Warning: rFID computation failed: {e}")
                self._fid, self._feats = False, ([], [])

    @torch.no_grad()
    def add(self, real, recon):
        if recon is None:
            return 0
        take, segs = self.planner.add(real.size(0))
        for _, lo, hi, pos in segs:
            if pos == 0 and hi - lo == self.chunk:  # a whole chunk inside this batch: no staging copy
                self._score(real[lo:hi], recon[lo:hi])
                continue
            if self._stage is None:
                shape = (self.chunk,) + tuple(real.shape[1:])
                self._stage = (torch.empty(shape, dtype=torch.float32, device=self.device),
                               torch.empty(shape, dtype=torch.float32, device=self.device))
            self._stage[0][pos: pos + hi - lo].copy_(real[lo:hi])
            self._stage[1][pos: pos + hi - lo].copy_(recon[lo:hi])
            self._fill = pos + hi - lo
            if self._fill == self.chunk:
                self._score(self._stage[0], self._stage[1])
                self._fill = 0
        return take

    def result(self):
        """Scores a partial last chunk, then reads every chunk's (ssim, psnr[, lpips]) with one host copy: the unweighted means
        over chunks of main.py:362-367."""
        if self._fill > 0:
            self._score(self._stage[0][: self._fill], self._stage[1][: self._fill])
            self._fill = 0
        out = dict(NAN_RESULT)
        if self._outs:
            vals = torch.stack(self._outs).cpu().double().numpy()
            out["ssim"] = float(np.mean(vals[:, 0]))
            out["psnr"] = float(np.mean(vals[:, 1]))
            if vals.shape[1] > 2:
                out["lpips"] = float(np.mean(vals[:, 2]))
        if self._fid and self.count >= 2:
            out["rfid"] = fid_from_features(torch.cat(self._feats[0]), torch.cat(self._feats[1]))
        if self._fid:
            release_inception_buffers(self.device)
        return out


# ---- hypervolume -------------------------------------------------------------------------------------------------------
def hv_ref_point(objective_keys, args):
    """main.py:681-689: a dict maps objective names to values (1.1 where absent); a list must match the objective count;
    anything else gives 1.1 for every objective."""
    keys = list(objective_keys)
    ref = getattr(args, "hv_ref", None)
    if ref is not None:
        if isinstance(ref, dict):
            return [float(ref.get(k, 1.1)) for k in keys]
        if isinstance(ref, (list, tuple)) and len(ref) == len(keys):
            return [float(v) for v in ref]
    return [1.1] * len(keys)


def build_hv_indicator(objective_keys, args):
    """main.py:659-692.  None for fewer than two objectives, else a callable giving the hypervolume dominated by one point
    (an array of shape (K,) or (1, K)) up to the reference point: prod(r - x) if x <= r in every objective, else 0 -- pymoo's
    HV(ref_point)(point) for a single point."""
    keys = list(objective_keys)
    if len(keys) < 2:
        return None
    ref = np.asarray(hv_ref_point(keys, args), dtype=np.float64)

    def hv(point):
        x = np.asarray(point, dtype=np.float64).reshape(-1, len(keys))
        if x.shape[0] != 1:
            raise ValueError("the closed form covers one point (what the training loop passes)")
        x = x[0]
        if not np.all(x <= ref):
            return 0.0
        return float(math.prod((ref - x).tolist()))

    hv.ref_point = ref
    return hv

"""Reconstruction metrics and the hypervolume of the objective vector (reference utils/metrics.py:14-203, main.py:335-463,
:659-692) on the HIP path.

`ssim` / `psnr` / `ssnr` keep the reference's signatures, return types and empty-input rules; each call is one chunk: its
[-1, 1] -> [0, 1] decision is taken over the whole input, as the reference's functions take it.  The arithmetic is one
C-ABI call (include/movae.h: movae_recon_metrics, three launches, no host read): the min-reduction that decides the
normalisation, the fused SSIM / MSE / signal-variance pass, and a fixed-order finalize.

`ReconMetricAccumulator` is the collection of main.py:376-463 without the host copies: (real, recon) pairs are taken batch by
batch up to `max_samples`, cut into the reference's 128-sample chunks (the chunks of the concatenated collection, so they
straddle loader batches), and each chunk is scored on the device as soon as it is complete.  `result()` is the one host read.

`build_hv_indicator` gives pymoo's HV for the single point the reference passes it, in closed form (pymoo is not needed).
"""
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
    """(real, recon) batches -> the reference's rFID / PSNR / SSIM / LPIPS dict (rFID and LPIPS need pretrained networks: NaN,
    as the reference gives when it cannot load them).  At most one chunk is staged on the device (a chunk that lies inside
    one batch is scored straight from the batch's tensors); every chunk is scored when it completes and its ssim / psnr stay
    on the device until result()."""

    def __init__(self, device, max_samples, chunk=CHUNK, window_size=11):
        _check_window(window_size)
        self.device = torch.device(device)
        self.planner = ChunkPlanner(max_samples, chunk)
        self.chunk, self.window_size = int(chunk), window_size
        self._stage = None  # (real, recon) NCHW float32 [chunk, C, H, W]
        self._fill = 0
        self._outs = []

    @property
    def full(self):
        return self.planner.full

    @property
    def count(self):
        return self.planner.seen

    def _score(self, real, recon):
        self._outs.append(_run(real, recon, self.window_size)[:2])

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
        """Scores a partial last chunk, then reads every chunk's (ssim, psnr) with one host copy: the unweighted means over
        chunks of main.py:367-370."""
        if self._fill > 0:
            self._score(self._stage[0][: self._fill], self._stage[1][: self._fill])
            self._fill = 0
        out = dict(NAN_RESULT)
        if self._outs:
            vals = torch.stack(self._outs).cpu().double().numpy()
            out["ssim"] = float(np.mean(vals[:, 0]))
            out["psnr"] = float(np.mean(vals[:, 1]))
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

"""Cached ancestral sampling for the PixelCNN priors: one launch per code instead of one full-grid forward per code.

PixelCNN.sample (the reference's pixelcnn_prior.py:323-349) runs forward_nhwc over the whole [B,H,W] grid for each of the H*W
positions and keeps one pixel's logits.  The network is causal, so the activations a layer needs at (i, j) were computed at
earlier raster positions and never change: CachedPixelCNNSampler keeps the input grid h0 = embedding(code) ++ condition and every
block's conv1 output on the device and computes one position of every sample per launch (csrc/prior_sample.hip), the categorical
draw included.  Under teacher forcing its logits are the full forward's logits at every position
(tests/test_prior_cached_sampling.py).

The draws are the inverse CDF at u = 24 bits of Philox4x32-10, keyed on (seed, draw number, absolute sample index, raster index):
they differ from torch.multinomial's for the same seed, and a sample does not depend on the batch it is drawn in."""
import torch
import torch.nn.functional as F

from . import ops

#: what csrc/prior_sample.hip supports (include/movae.h: movae_prior_sample_step)
MAX_HIDDEN, MAX_INPUT_CHANNELS, MAX_CODES, MAX_KERNEL = 256, 256, 2048, 7
#: h0 and the blocks' caches of one chunk of the batch stay under this many bytes; a larger batch is sampled in chunks
MAX_CACHE_BYTES = 4 << 30


def _pad4(n):
    return (n + 3) & ~3


def _matrix(conv, taps):
    """[Co,Ci,kh,kw] weight -> [taps * Ci, pad4(Co)] over the first `taps` taps in raster order (the causal ones), and the bias."""
    w = conv.weight.detach()
    co, ci = w.shape[:2]
    m = w.permute(2, 3, 1, 0).reshape(-1, ci, co)[:taps].reshape(taps * ci, co)
    b = conv.bias.detach() if conv.bias is not None else torch.zeros(co, dtype=w.dtype, device=w.device)
    return F.pad(m, (0, _pad4(co) - co)), F.pad(b, (0, _pad4(co) - co))


class CachedPixelCNNSampler:
    """sampler = CachedPixelCNNSampler(prior); codes = sampler.run(B, H, W) -- for a models.pixelcnn_prior.PixelCNN."""

    def __init__(self, prior):
        for name in ("embedding", "conv_in", "res_blocks", "conv_out"):
            if not hasattr(prior, name) or hasattr(prior, "blocks"):
                raise TypeError("CachedPixelCNNSampler samples a PixelCNN (embedding, conv_in, res_blocks, conv_out); "
                                f"got {type(prior).__name__}")
        self.prior = prior
        self.draws = 0  # the draw number of the next run (advances once per run)
        self.dims()

    def dims(self):
        """(D0, E, C, L, K, ks) of the prior as it is now; ValueError names the limit an unsupported shape breaks."""
        p = self.prior
        e, k = p.embedding.weight.shape[1], p.embedding.weight.shape[0]
        d0, c, ks = p.conv_in.in_channels, p.conv_in.out_channels, p.conv_in.kernel_size
        if c % 2 or not 2 <= c <= MAX_HIDDEN:
            raise ValueError(f"cached sampling needs an even hidden_channels <= {MAX_HIDDEN}, got {c}")
        if not e <= d0 <= MAX_INPUT_CHANNELS:
            raise ValueError(f"cached sampling needs embedding_dim + conditional_channels <= {MAX_INPUT_CHANNELS}, got {d0}")
        if k > MAX_CODES:
            raise ValueError(f"cached sampling needs num_embeddings <= {MAX_CODES}, got {k}")
        if ks % 2 == 0 or ks > MAX_KERNEL or p.conv_in.padding != ks // 2 or p.conv_in.stride != 1:
            raise ValueError(f"cached sampling needs an odd conv_in kernel_size <= {MAX_KERNEL} with 'same' padding, got {ks}")
        for blk in p.res_blocks:
            if blk.conv2.kernel_size != 3 or blk.conv2.padding != 1:
                raise ValueError(f"cached sampling needs 3x3 gated blocks, got kernel_size {blk.conv2.kernel_size}")
        return d0, e, c, len(p.res_blocks), k, ks

    @torch.no_grad()
    def pack_weights(self):
        """The one contiguous fp32 buffer the step kernel reads, in its layout (include/movae.h), from the parameters as they are
        now: causal taps only, after the masks have been applied in place like a forward applies them."""
        p = self.prior
        d0, e, c, layers, k, ks = self.dims()
        ops.mask_weight_(p.conv_in.weight, p.conv_in.mask)
        parts = list(_matrix(p.conv_in, (ks // 2) * ks + ks // 2))
        for blk in p.res_blocks:
            ops.mask_weight_(blk.conv2.weight, blk.conv2.mask)
            parts += _matrix(blk.conv1, 1)
            parts += _matrix(blk.conv2, 5)
            (gw, gb), (fw, fb) = _matrix(blk.conv_gate, 1), _matrix(blk.conv_feature, 1)
            parts += [torch.cat([gw, fw], dim=1), torch.cat([gb, fb])]
        parts += _matrix(p.conv_out[1], 1)
        parts += _matrix(p.conv_out[3], 1)
        parts.append(p.embedding.weight.detach())
        wpack = torch.cat([t.reshape(-1).float() for t in parts])
        want = ops.prior_sample_pack_floats(d0, e, c, layers, k, ks)
        assert wpack.numel() == want, f"packed {wpack.numel()} floats, the kernel's layout has {want}"
        return wpack

    @torch.no_grad()
    def run(self, batch_size, height, width, condition=None, temperature=1.0, seed=None, forced=None, uniforms=None, return_logits=False):
        """Codes [B,H,W] int64 (and the raw NHWC logits [B,H,W,K] of every position when return_logits is set).

        condition: NCHW [B, conditional_channels, H, W], as for PixelCNN.sample.  seed: None takes torch.cuda.initial_seed(); the
        draw number is self.draws, which advances once per run.  forced [B,H,W] int64: these codes instead of the draws (teacher
        forcing).  uniforms [B,H,W] fp32: these u in [0, 1) instead of Philox."""
        p = self.prior
        d0, e, c, layers, k, ks = self.dims()
        B, H, W = int(batch_size), int(height), int(width)
        if min(B, H, W) < 1:
            raise ValueError(f"cached sampling needs batch_size, height, width >= 1, got {(B, H, W)}")
        if not temperature > 0:
            raise ValueError(f"temperature must be positive, got {temperature}")
        dev = p.embedding.weight.device
        cond = None
        if condition is not None:
            cond = ops.to_nhwc(condition)
        if (0 if cond is None else cond.shape[-1]) != d0 - e or (cond is not None and tuple(cond.shape[:3]) != (B, H, W)):
            raise ValueError(f"the prior takes a condition of {d0 - e} channels on the {(B, H, W)} grid, got "
                             f"{None if condition is None else tuple(condition.shape)}")
        if forced is not None:
            forced = forced.to(device=dev, dtype=torch.int64).contiguous()
        if uniforms is not None:
            uniforms = uniforms.to(device=dev, dtype=torch.float32).contiguous()
        for name, t in (("forced", forced), ("uniforms", uniforms)):
            if t is not None and tuple(t.shape) != (B, H, W):
                raise ValueError(f"{name} must be [B,H,W] = {(B, H, W)}, got {tuple(t.shape)}")
        wpack = self.pack_weights()
        seed = (torch.cuda.initial_seed() if seed is None else int(seed)) & 0xFFFFFFFFFFFFFFFF
        draw = self.draws
        self.draws += 1
        codes = torch.empty((B, H, W), dtype=torch.int64, device=dev)
        logits = torch.empty((B, H, W, k), dtype=torch.float32, device=dev) if return_logits else None
        chunk = max(1, MAX_CACHE_BYTES // (4 * H * W * (d0 + layers * (c // 2))))
        for b0 in range(0, B, chunk):
            b1 = min(B, b0 + chunk)
            h0 = torch.zeros((b1 - b0, H, W, d0), dtype=torch.float32, device=dev)
            if cond is not None:
                h0[..., e:] = cond[b0:b1]
            acache = torch.empty((layers, b1 - b0, H, W, c // 2), dtype=torch.float32, device=dev) if layers else None
            part = [None if t is None else t[b0:b1] for t in (forced, uniforms, logits)]
            for i in range(H):
                for j in range(W):
                    ops.prior_sample_step(wpack, h0, acache, codes[b0:b1], (e, c, layers, k, ks), i, j, 1.0 / temperature, seed, draw,
                                          sample_base=b0, forced=part[0], uniforms=part[1], logits_out=part[2])
        return (codes, logits) if return_logits else codes

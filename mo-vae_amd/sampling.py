"""Cached ancestral sampling for the PixelCNN and PixelSNAIL priors: one launch per code instead of one full-grid forward per code.

PixelCNN.sample (the reference's pixelcnn_prior.py:323-349) runs forward_nhwc over the whole [B,H,W] grid for each of the H*W
positions and keeps one pixel's logits.  The network is causal, so the activations a layer needs at (i, j) were computed at
earlier raster positions and never change: CachedPixelCNNSampler keeps the input grid h0 = embedding(code) ++ condition and every
block's conv1 output on the device and computes one position of every sample per launch (csrc/prior_sample.hip), the categorical
draw included.  Under teacher forcing its logits are the full forward's logits at every position
(tests/test_prior_cached_sampling.py).

The draws are the inverse CDF at u = 24 bits of Philox4x32-10, keyed on (seed, draw number, absolute sample index, raster index):
they differ from torch.multinomial's for the same seed, and a sample does not depend on the batch it is drawn in.

CachedPixelSNAILSampler does the same for PixelSNAIL: its step also keeps the K and V rows of every attention layer and attends
over them (tests/test_pixelsnail_cached_sampling.py)."""
import torch
import torch.nn.functional as F

from . import ops

#: what csrc/prior_sample.hip supports (include/movae.h: movae_prior_sample_step)
MAX_HIDDEN, MAX_INPUT_CHANNELS, MAX_CODES, MAX_KERNEL = 256, 256, 2048, 7
#: and of the PixelSNAIL step's attention (movae_prior_snail_sample_step): head_dim, num_heads * head_dim
MAX_HEAD_DIM, MAX_PROJ = 64, 256
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


class _CachedSampler:
    """What the cached samplers share: the checks and the raster loop of run().  A subclass gives dims(), pack_weights(), the cache
    floats of one code (_cache_floats), the buffers of a chunk (_buffers) and the launch of one position (_step)."""

    def __init__(self, prior):
        self.prior = prior
        self.draws = 0  # the draw number of the next run (advances once per run)
        self.dims()

    @torch.no_grad()
    def run(self, batch_size, height, width, condition=None, temperature=1.0, seed=None, forced=None, uniforms=None, return_logits=False):
        """Codes [B,H,W] int64 (and the raw NHWC logits [B,H,W,K] of every position when return_logits is set).

        condition: NCHW [B, conditional_channels, H, W], as for the prior's sample().  seed: None takes torch.cuda.initial_seed(); the
        draw number is self.draws, which advances once per run.  forced [B,H,W] int64: these codes instead of the draws (teacher
        forcing).  uniforms [B,H,W] fp32: these u in [0, 1) instead of Philox."""
        p = self.prior
        dims = self.dims()
        d0, e, k = dims[0], dims[1], p.embedding.weight.shape[0]
        B, H, W = int(batch_size), int(height), int(width)
        if min(B, H, W) < 1:
            raise ValueError(f"cached sampling needs batch_size, height, width >= 1, got {(B, H, W)}")
        if not temperature > 0:
            raise ValueError(f"temperature must be positive, got {temperature}")
        dev = p.embedding.weight.device
        cond = None
        if condition is not None:
            cond = ops.to_nhwc(condition)
        nc = d0 - e - self.EXTRA_CHANNELS
        if (0 if cond is None else cond.shape[-1]) != nc or (cond is not None and tuple(cond.shape[:3]) != (B, H, W)):
            raise ValueError(f"the prior takes a condition of {nc} channels on the {(B, H, W)} grid, got "
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
        chunk = max(1, MAX_CACHE_BYTES // (4 * H * W * self._cache_floats(dims)))
        for b0 in range(0, B, chunk):
            b1 = min(B, b0 + chunk)
            bufs = self._buffers(dims, b1 - b0, H, W, None if cond is None else cond[b0:b1], dev)
            part = [None if t is None else t[b0:b1] for t in (forced, uniforms, logits)]
            for i in range(H):
                for j in range(W):
                    self._step(wpack, bufs, codes[b0:b1], dims, i, j, 1.0 / temperature, seed, draw, sample_base=b0, forced=part[0],
                               uniforms=part[1], logits_out=part[2])
        return (codes, logits) if return_logits else codes


def _gated_parts(blk):
    """The packed sections of one GatedResBlock: conv1, conv2 over its 5 causal taps (masked in place first), gate ++ feature."""
    ops.mask_weight_(blk.conv2.weight, blk.conv2.mask)
    (gw, gb), (fw, fb) = _matrix(blk.conv_gate, 1), _matrix(blk.conv_feature, 1)
    return [*_matrix(blk.conv1, 1), *_matrix(blk.conv2, 5), torch.cat([gw, fw], dim=1), torch.cat([gb, fb])]


def _check_common(c, e, d0, k, conv_in, gated, what):
    ks = conv_in.kernel_size
    if c % 2 or not 2 <= c <= MAX_HIDDEN:
        raise ValueError(f"cached sampling needs an even hidden_channels <= {MAX_HIDDEN}, got {c}")
    if not e <= d0 <= MAX_INPUT_CHANNELS:
        raise ValueError(f"cached sampling needs {what} <= {MAX_INPUT_CHANNELS}, got {d0}")
    if k > MAX_CODES:
        raise ValueError(f"cached sampling needs num_embeddings <= {MAX_CODES}, got {k}")
    if ks % 2 == 0 or ks > MAX_KERNEL or conv_in.padding != ks // 2 or conv_in.stride != 1:
        raise ValueError(f"cached sampling needs an odd conv_in kernel_size <= {MAX_KERNEL} with 'same' padding, got {ks}")
    for blk in gated:
        if blk.conv2.kernel_size != 3 or blk.conv2.padding != 1:
            raise ValueError(f"cached sampling needs 3x3 gated blocks, got kernel_size {blk.conv2.kernel_size}")


class CachedPixelCNNSampler(_CachedSampler):
    """sampler = CachedPixelCNNSampler(prior); codes = sampler.run(B, H, W) -- for a models.pixelcnn_prior.PixelCNN."""

    EXTRA_CHANNELS = 0  # of h0, between the embedding and the condition

    def __init__(self, prior):
        for name in ("embedding", "conv_in", "res_blocks", "conv_out"):
            if not hasattr(prior, name) or hasattr(prior, "blocks"):
                raise TypeError("CachedPixelCNNSampler samples a PixelCNN (embedding, conv_in, res_blocks, conv_out); "
                                f"got {type(prior).__name__}")
        super().__init__(prior)

    def dims(self):
        """(D0, E, C, L, K, ks) of the prior as it is now; ValueError names the limit an unsupported shape breaks."""
        p = self.prior
        e, k = p.embedding.weight.shape[1], p.embedding.weight.shape[0]
        d0, c, ks = p.conv_in.in_channels, p.conv_in.out_channels, p.conv_in.kernel_size
        _check_common(c, e, d0, k, p.conv_in, p.res_blocks, "embedding_dim + conditional_channels")
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
            parts += _gated_parts(blk)
        parts += _matrix(p.conv_out[1], 1)
        parts += _matrix(p.conv_out[3], 1)
        parts.append(p.embedding.weight.detach())
        wpack = torch.cat([t.reshape(-1).float() for t in parts])
        want = ops.prior_sample_pack_floats(d0, e, c, layers, k, ks)
        assert wpack.numel() == want, f"packed {wpack.numel()} floats, the kernel's layout has {want}"
        return wpack

    def _cache_floats(self, dims):
        d0, _, c, layers, _, _ = dims
        return d0 + layers * (c // 2)

    def _buffers(self, dims, b, H, W, cond, dev):
        d0, e, c, layers, _, _ = dims
        h0 = torch.zeros((b, H, W, d0), dtype=torch.float32, device=dev)
        if cond is not None:
            h0[..., e:] = cond
        return h0, (torch.empty((layers, b, H, W, c // 2), dtype=torch.float32, device=dev) if layers else None)

    def _step(self, wpack, bufs, codes, dims, i, j, inv_temperature, seed, draw, **kw):
        ops.prior_sample_step(wpack, bufs[0], bufs[1], codes, dims[1:], i, j, inv_temperature, seed, draw, **kw)


class CachedPixelSNAILSampler(_CachedSampler):
    """sampler = CachedPixelSNAILSampler(prior); codes = sampler.run(B, H, W) -- for a models.pixelcnn_prior.PixelSNAIL.  Besides
    h0 (embedding ++ the 2 position channels ++ condition) and the gated blocks' conv1 outputs it keeps every attention layer's K and
    V rows, kv [blocks][B][H*W][2 * heads * head_dim].  Eval mode whatever the modules' `training` flag says: no dropout."""

    EXTRA_CHANNELS = 2  # the row / column coordinates

    def __init__(self, prior):
        ok = all(hasattr(prior, name) for name in ("embedding", "conv_in", "blocks", "conv_out", "_pos_encoding"))
        if not ok or not all(hasattr(blk, "attention") and hasattr(blk, "res_blocks") and hasattr(blk, "out_conv") for blk in prior.blocks):
            raise TypeError("CachedPixelSNAILSampler samples a PixelSNAIL (embedding, conv_in, blocks with attention, conv_out); "
                            f"got {type(prior).__name__}")
        super().__init__(prior)

    def dims(self):
        """(D0, E, C, blocks, res_blocks, heads, head_dim, K, ks) of the prior as it is now; ValueError names the limit an unsupported
        shape breaks."""
        p = self.prior
        e, k = p.embedding.weight.shape[1], p.embedding.weight.shape[0]
        d0, c, ks = p.conv_in.in_channels, p.conv_in.out_channels, p.conv_in.kernel_size
        _check_common(c, e + 2, d0, k, p.conv_in, [g for blk in p.blocks for g in blk.res_blocks],
                      "embedding_dim + 2 + conditional_channels")
        shapes = {(len(blk.res_blocks), blk.attention.num_heads, blk.attention.head_dim) for blk in p.blocks}
        if len(shapes) > 1:
            raise ValueError(f"cached sampling needs PixelSNAIL blocks of one shape, got (res_blocks, heads, head_dim) in {sorted(shapes)}")
        nr, heads, hd = shapes.pop() if shapes else (0, 1, 1)
        if not 1 <= hd <= MAX_HEAD_DIM:
            raise ValueError(f"cached sampling needs an attention head_dim <= {MAX_HEAD_DIM}, got {hd}")
        if heads * hd > MAX_PROJ:
            raise ValueError(f"cached sampling needs num_heads * head_dim <= {MAX_PROJ}, got {heads * hd}")
        return d0, e, c, len(p.blocks), nr, heads, hd, k, ks

    @torch.no_grad()
    def pack_weights(self):
        """As CachedPixelCNNSampler.pack_weights; per PixelSNAILBlock its gated blocks, q ++ k ++ v side by side, out_proj, out_conv."""
        p = self.prior
        dims = self.dims()
        ks = dims[-1]
        ops.mask_weight_(p.conv_in.weight, p.conv_in.mask)
        parts = list(_matrix(p.conv_in, (ks // 2) * ks + ks // 2))
        for blk in p.blocks:
            for g in blk.res_blocks:
                parts += _gated_parts(g)
            att = blk.attention
            qkv = [_matrix(m, 1) for m in (att.q_proj, att.k_proj, att.v_proj)]
            parts += [torch.cat([w for w, _ in qkv], dim=1), torch.cat([b for _, b in qkv])]
            parts += _matrix(att.out_proj, 1)
            parts += _matrix(blk.out_conv, 1)
        parts += _matrix(p.conv_out[1], 1)
        parts += _matrix(p.conv_out[3], 1)
        parts.append(p.embedding.weight.detach())
        wpack = torch.cat([t.reshape(-1).float() for t in parts])
        want = ops.prior_snail_sample_pack_floats(*dims)
        assert wpack.numel() == want, f"packed {wpack.numel()} floats, the kernel's layout has {want}"
        return wpack

    def _cache_floats(self, dims):
        d0, _, c, nb, nr, heads, hd, _, _ = dims
        return d0 + nb * nr * (c // 2) + nb * 2 * heads * hd

    def _buffers(self, dims, b, H, W, cond, dev):
        d0, e, c, nb, nr, heads, hd, _, _ = dims
        h0 = torch.zeros((b, H, W, d0), dtype=torch.float32, device=dev)
        h0[..., e:e + 2] = self.prior._pos_encoding(1, H, W, dev)  # the numbers the forward concatenates
        if cond is not None:
            h0[..., e + 2:] = cond
        acache = torch.empty((nb * nr, b, H, W, c // 2), dtype=torch.float32, device=dev) if nb * nr else None
        kv = torch.empty((nb, b, H * W, 2 * heads * hd), dtype=torch.float32, device=dev) if nb else None
        return h0, acache, kv

    def _step(self, wpack, bufs, codes, dims, i, j, inv_temperature, seed, draw, **kw):
        ops.prior_snail_sample_step(wpack, bufs[0], bufs[1], bufs[2], codes, dims[1:], i, j, inv_temperature, seed, draw, **kw)

"""PixelCNN priors over the discrete VQ code grids on the HIP kernels -- drop-in for the reference's
models/pixelcnn_prior.py:25-54 (MaskedConv2d), :57-92 (GatedResBlock), :262-349 (PixelCNN) and :352-421 (HierarchicalPixelCNN):
same constructor signatures, state_dict keys (incl. the `mask` buffers) and init sequence, forward(x[B,H,W] int64) -> logits
[B, K, H, W] (a zero-copy NCHW view of the NHWC logits the kernels write).  PixelSNAIL (:95-259) and HierarchicalPixelSNAIL
(:434-555) add causal self-attention, which runs on the fused kernels of csrc/attention.hip (ops.causal_attention); prior.py builds
them with build_pixelsnail_prior, while `--prior_type pixelsnail` on the command line is still refused by name.

Every convolution runs on the implicit-GEMM kernels; the embedding gather, the gated combine, the weight mask and the
cross-entropy are csrc/prior.hip.  Activations stay NHWC: nn.Embedding of a [B,H,W] grid IS the NHWC activation, and the
NHWC logits viewed as [B*H*W, K] are exactly the matrix F.cross_entropy is handed after the reference's permute + reshape."""
import torch
import torch.nn as tnn

from .. import nn as mnn
from .. import ops
from ._base import nchw_view


class MaskedConv2d(mnn.Conv2d):
    """pixelcnn_prior.py:25-54.  The mask multiplies the weight IN PLACE before each forward (so masked entries of the
    parameter are zero whenever it is used, whatever the optimizer wrote there in between)."""

    def __init__(self, mask_type, cin, cout, k, stride=1, padding=0, bias=True):
        super().__init__(cin, cout, k, stride=stride, padding=padding, bias=bias)
        assert mask_type in ("A", "B"), "mask_type must be 'A' or 'B'"
        mask = torch.zeros(cout, cin, k, k)
        mask[:, :, : k // 2, :] = 1.0
        mask[:, :, k // 2, : k // 2] = 1.0
        if mask_type == "B":
            mask[:, :, k // 2, k // 2] = 1.0
        self.register_buffer("mask", mask.contiguous(memory_format=torch.channels_last))  # the weight's memory layout
        self.mask_type = mask_type

    def forward(self, x, act=None, feeds_batchnorm=False):
        ops.mask_weight_(self.weight, self.mask)
        return super().forward(x, act, feeds_batchnorm)


class GatedResBlock(tnn.Module):
    """pixelcnn_prior.py:57-92: 1x1 -> ReLU -> masked-B 3x3 -> ReLU -> sigmoid(1x1) * tanh(1x1) + residual."""

    def __init__(self, channels, kernel_size=3):
        super().__init__()
        self.conv1 = mnn.Conv2d(channels, channels // 2, 1)
        self.conv2 = MaskedConv2d("B", channels // 2, channels // 2, kernel_size, padding=kernel_size // 2)
        self.conv_gate = mnn.Conv2d(channels // 2, channels, 1)
        self.conv_feature = mnn.Conv2d(channels // 2, channels, 1)

    def forward(self, x):
        out = self.conv2(self.conv1(x, "relu"), "relu")
        return ops.gated_residual(x, self.conv_gate(out, "sigmoid"), self.conv_feature(out, "tanh"))


class _OutHead(mnn.Stack):
    """nn.Sequential(ReLU, Conv1x1, ReLU, Conv1x1) with the reference's child indices 0..3 (pixelcnn_prior.py:300-305)."""

    def __init__(self, hidden, out):
        super().__init__(mnn.ReLU(), mnn.Conv2d(hidden, hidden, 1), mnn.ReLU(), mnn.Conv2d(hidden, out, 1))


class Embedding(tnn.Module):
    """nn.Embedding(K, D) with its default N(0, 1) init."""

    def __init__(self, K, D):
        super().__init__()
        ref = tnn.Embedding(K, D)
        self.weight = tnn.Parameter(ref.weight.detach().clone())
        self.num_embeddings, self.embedding_dim = K, D

    def forward(self, idx):
        return ops.embedding(idx, self.weight)


class PixelCNN(tnn.Module):
    """pixelcnn_prior.py:262-349."""

    def __init__(self, num_embeddings, embedding_dim=64, hidden_channels=128, num_layers=15, kernel_size=7, conditional_channels=0):
        super().__init__()
        self.num_embeddings, self.embedding_dim = num_embeddings, embedding_dim
        self.embedding = Embedding(num_embeddings, embedding_dim)
        self.conv_in = MaskedConv2d("A", embedding_dim + conditional_channels, hidden_channels, kernel_size, padding=kernel_size // 2)
        self.res_blocks = tnn.ModuleList([GatedResBlock(hidden_channels) for _ in range(num_layers)])
        self.conv_out = _OutHead(hidden_channels, num_embeddings)

    def forward_nhwc(self, x, condition=None):
        """x [B, H, W] int64, condition NHWC [B, H, W, C] or None -> NHWC logits [B, H, W, K]."""
        h = self.embedding(x)
        if condition is not None:
            h = ops.concat_channels(h, condition)
        h = self.conv_in(h)
        for blk in self.res_blocks:
            h = blk(h)
        return self.conv_out(h)

    def forward(self, x, condition=None):
        if condition is not None:
            condition = ops.to_nhwc(condition)
        return nchw_view(self.forward_nhwc(x, condition))

    def loss(self, x, condition=None):
        """F.cross_entropy(logits.permute(0,2,3,1).reshape(-1, K), x.reshape(-1)) (main.py:1003-1006)."""
        logits = self.forward_nhwc(x, condition)
        return ops.cross_entropy(logits.reshape(-1, self.num_embeddings), x.reshape(-1))

    @torch.no_grad()
    def sample(self, batch_size, height, width, device, condition=None, temperature=1.0, cached=False):
        """Raster-scan ancestral sampling (pixelcnn_prior.py:323-349); the categorical draw uses torch's device generator.
        cached=True: one launch per code on the cached activations (sampling.CachedPixelCNNSampler) instead of one full forward per
        code; its draws come from Philox under torch.cuda.initial_seed(), so they differ from the full path's for the same seed."""
        self.eval()
        if cached:
            return self.cached_sampler().run(batch_size, height, width, condition=condition, temperature=temperature)
        samples = torch.zeros(batch_size, height, width, dtype=torch.long, device=device)
        cond = ops.to_nhwc(condition) if condition is not None else None
        for i in range(height):
            for j in range(width):
                logits = self.forward_nhwc(samples, cond)[:, i, j, :] / temperature
                probs = torch.softmax(logits, dim=1)
                samples[:, i, j] = torch.multinomial(probs, 1).squeeze(-1)
        return samples

    def cached_sampler(self):
        """This model's CachedPixelCNNSampler, kept so that its draw counter advances from one sample() call to the next."""
        from ..sampling import CachedPixelCNNSampler

        s = self.__dict__.get("_cached_sampler")
        if s is None:
            s = self.__dict__["_cached_sampler"] = CachedPixelCNNSampler(self)
        return s

    def total_trainable_params(self):
        return sum(p.numel() for p in self.parameters() if p.requires_grad)


class HierarchicalPixelCNN(tnn.Module):
    """pixelcnn_prior.py:352-421: P(z_top) and P(z_bottom | upsampled embedding of z_top)."""

    def __init__(self, num_embeddings, embedding_dim=64, hidden_channels=128, num_layers=15):
        super().__init__()
        self.num_embeddings, self.embedding_dim = num_embeddings, embedding_dim
        self.prior_top = PixelCNN(num_embeddings, embedding_dim, hidden_channels, num_layers)
        self.embedding_top = Embedding(num_embeddings, embedding_dim)
        self.upsample_top = mnn.ConvTranspose2d(embedding_dim, embedding_dim, 4, stride=2, padding=1)
        self.prior_bottom = PixelCNN(num_embeddings, embedding_dim, hidden_channels, num_layers, conditional_channels=embedding_dim)

    def _condition(self, z_top):
        return self.upsample_top(self.embedding_top(z_top))  # NHWC

    def forward_top(self, z_top):
        return self.prior_top(z_top)

    def forward_bottom(self, z_bottom, z_top):
        return nchw_view(self.prior_bottom.forward_nhwc(z_bottom, self._condition(z_top)))

    def forward(self, z_top, z_bottom):
        return {"logits_top": self.forward_top(z_top), "logits_bottom": self.forward_bottom(z_bottom, z_top)}

    def loss_function(self, z_top, z_bottom):
        loss_top = self.prior_top.loss(z_top)
        loss_bottom = self.prior_bottom.loss(z_bottom, self._condition(z_top))
        return {"loss_top": loss_top, "loss_bottom": loss_bottom, "total_loss": loss_top + loss_bottom}

    @torch.no_grad()
    def sample(self, batch_size, top_shape, bottom_shape, device, temperature=1.0, cached=False):
        """cached: both levels through PixelCNN.sample(cached=True); the upsampled top embedding is the bottom level's condition."""
        self.eval()
        z_top = self._sample_top(batch_size, top_shape, device, temperature, cached)
        cond = nchw_view(self._condition(z_top))
        z_bottom = self.prior_bottom.sample(batch_size, bottom_shape[0], bottom_shape[1], device, condition=cond, temperature=temperature,
                                            cached=cached)
        return z_top, z_bottom

    def _sample_top(self, batch_size, top_shape, device, temperature, cached):
        return self.prior_top.sample(batch_size, top_shape[0], top_shape[1], device, temperature=temperature, cached=cached)

    @torch.no_grad()
    def sample_with_vqvae2(self, vqvae2_model, batch_size, device, temperature=1.0, cached=False):
        t, b = vqvae2_model.latent_spatial_dim_top, vqvae2_model.latent_spatial_dim_bottom
        z_top, z_bottom = self.sample(batch_size, (t, t), (b, b), device, temperature, cached=cached)
        return vqvae2_model.decode_code(z_top, z_bottom)

    def total_trainable_params(self):
        return sum(p.numel() for p in self.parameters() if p.requires_grad)


class CausalAttention2d(tnn.Module):
    """pixelcnn_prior.py:95-135 on NHWC activations: three 1x1 projections, the fused causal attention (ops.causal_attention: no
    [L, L] matrix) and out_proj, which reads the attention output in the reference's channel order d * heads + h.

    Dropout (the reference's nn.Dropout on the probabilities) is drawn inside the kernels from (seed, draw): seed is
    torch.cuda.initial_seed(), draw combines the module's index in its model (`stream`) with a host counter that advances once per
    training-mode forward, so the same torch.manual_seed gives the same masks and nothing is drawn from torch's generators."""

    def __init__(self, channels, num_heads=8, head_dim=None, dropout=0.1):
        super().__init__()
        self.num_heads = num_heads
        self.head_dim = head_dim or (channels // num_heads)
        assert channels % num_heads == 0 or head_dim is not None, "channels must be divisible by num_heads"
        self.proj_dim = self.head_dim * num_heads
        self.q_proj = mnn.Conv2d(channels, self.proj_dim, 1)
        self.k_proj = mnn.Conv2d(channels, self.proj_dim, 1)
        self.v_proj = mnn.Conv2d(channels, self.proj_dim, 1)
        self.out_proj = mnn.Conv2d(self.proj_dim, channels, 1)
        self.dropout = tnn.Dropout(dropout)  # holds p; never called (the kernels apply it)
        self.stream = 0  # set by PixelSNAIL: distinct dropout streams per block
        self.draws = 0

    def forward(self, x):
        p = self.dropout.p if self.training else 0.0
        seed = draw = 0
        if p > 0.0:
            seed, draw = torch.cuda.initial_seed(), (self.stream << 40) | self.draws
            self.draws += 1
        o = ops.causal_attention(self.q_proj(x), self.k_proj(x), self.v_proj(x), self.num_heads, p, seed, draw)
        return self.out_proj(o)


class PixelSNAILBlock(tnn.Module):
    """pixelcnn_prior.py:138-156: gated residual blocks, causal attention, out_conv(cat([x, attn])) + x."""

    def __init__(self, channels, num_res_blocks=2, num_heads=8, dropout=0.1):
        super().__init__()
        self.res_blocks = tnn.ModuleList([GatedResBlock(channels) for _ in range(num_res_blocks)])
        self.attention = CausalAttention2d(channels, num_heads=num_heads, dropout=dropout)
        self.out_conv = mnn.Conv2d(channels * 2, channels, 1)

    def forward(self, x):
        for blk in self.res_blocks:
            x = blk(x)
        return ops.add(self.out_conv(ops.concat_channels(x, self.attention(x))), x)


class PixelSNAIL(tnn.Module):
    """pixelcnn_prior.py:159-259."""

    def __init__(self, num_embeddings, embedding_dim=64, hidden_channels=128, num_blocks=8, num_res_blocks_per_layer=2, num_heads=8,
                 kernel_size=7, conditional_channels=0, dropout=0.1):
        super().__init__()
        self.num_embeddings, self.embedding_dim = num_embeddings, embedding_dim
        self.embedding = Embedding(num_embeddings, embedding_dim)
        self.conv_in = MaskedConv2d("A", embedding_dim + conditional_channels + 2, hidden_channels, kernel_size, padding=kernel_size // 2)
        self.blocks = tnn.ModuleList([PixelSNAILBlock(hidden_channels, num_res_blocks=num_res_blocks_per_layer, num_heads=num_heads,
                                                      dropout=dropout) for _ in range(num_blocks)])
        self.conv_out = _OutHead(hidden_channels, num_embeddings)
        for i, blk in enumerate(self.blocks):
            blk.attention.stream = i
        self._pos = {}

    def _pos_encoding(self, batch, height, width, device):
        """NHWC [B, H, W, 2] of the reference's row / column coordinates (:195-203), built once per shape."""
        key = (batch, height, width, str(device))
        pos = self._pos.get(key)
        if pos is None:
            coord_h = (torch.arange(height, dtype=torch.float32) - height / 2) / max(height, 1)
            coord_w = (torch.arange(width, dtype=torch.float32) - width / 2) / max(width, 1)
            pos = torch.stack([coord_h.view(height, 1).expand(height, width), coord_w.view(1, width).expand(height, width)], dim=-1)
            pos = self._pos[key] = pos.expand(batch, height, width, 2).contiguous().to(device)
        return pos

    def forward_nhwc(self, x, condition=None):
        """x [B, H, W] int64, condition NHWC [B, H, W, C] or None -> NHWC logits [B, H, W, K]."""
        B, H, W = x.shape
        h = ops.concat_channels(self.embedding(x), self._pos_encoding(B, H, W, x.device))
        if condition is not None:
            h = ops.concat_channels(h, condition)
        h = self.conv_in(h)
        for blk in self.blocks:
            h = ops.add(h, blk(h))
        return self.conv_out(h)

    forward = PixelCNN.forward
    loss = PixelCNN.loss

    def sample(self, batch_size, height, width, device, condition=None, temperature=1.0, cached=False):
        """cached="kv": one launch per code on the cached activations and the attention layers' K/V cache
        (sampling.CachedPixelSNAILSampler), with Philox inverse-CDF draws like PixelCNN's cached path.  Any other truthy value still
        raises: cached=True means the PixelCNN levels' sampler, which this model does not have."""
        if cached == "kv":
            self.eval()
            return self.cached_sampler().run(batch_size, height, width, condition=condition, temperature=temperature)
        if cached:
            raise NotImplementedError("PixelSNAIL.sample(cached=True): the attention K/V cache is not built on this path; cached=True "
                                      "covers PixelCNN and HierarchicalPixelCNN (sampling.CachedPixelCNNSampler).  Pass cached=\"kv\" "
                                      "for the K/V-cached sampler (sampling.CachedPixelSNAILSampler)")
        return PixelCNN.sample(self, batch_size, height, width, device, condition=condition, temperature=temperature)

    def cached_sampler(self):
        """This model's CachedPixelSNAILSampler, kept so that its draw counter advances from one sample() call to the next."""
        from ..sampling import CachedPixelSNAILSampler

        s = self.__dict__.get("_cached_sampler")
        if s is None:
            s = self.__dict__["_cached_sampler"] = CachedPixelSNAILSampler(self)
        return s

    total_trainable_params = PixelCNN.total_trainable_params


class HierarchicalPixelSNAIL(HierarchicalPixelCNN):
    """pixelcnn_prior.py:434-555: PixelSNAIL over the top codes, the conditional PixelCNN over the bottom codes."""

    def __init__(self, num_embeddings, embedding_dim=64, hidden_channels=128, num_blocks_top=8, num_res_blocks_per_layer=2, num_heads=8,
                 num_layers_bottom=15, dropout=0.1):
        tnn.Module.__init__(self)
        self.num_embeddings, self.embedding_dim = num_embeddings, embedding_dim
        self.prior_top = PixelSNAIL(num_embeddings=num_embeddings, embedding_dim=embedding_dim, hidden_channels=hidden_channels,
                                    num_blocks=num_blocks_top, num_res_blocks_per_layer=num_res_blocks_per_layer, num_heads=num_heads,
                                    dropout=dropout)
        self.embedding_top = Embedding(num_embeddings, embedding_dim)
        self.upsample_top = mnn.ConvTranspose2d(embedding_dim, embedding_dim, 4, stride=2, padding=1)
        self.prior_bottom = PixelCNN(num_embeddings, embedding_dim, hidden_channels, num_layers_bottom, conditional_channels=embedding_dim)

    def _sample_top(self, batch_size, top_shape, device, temperature, cached):
        """cached="kv": the PixelSNAIL top through its K/V-cached sampler.  Any other value: by full recompute, as before that sampler
        existed; the PixelCNN bottom, the expensive level, takes the cached path for every truthy `cached`."""
        return self.prior_top.sample(batch_size, top_shape[0], top_shape[1], device, temperature=temperature,
                                     cached="kv" if cached == "kv" else False)

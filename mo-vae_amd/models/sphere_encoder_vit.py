"""The ViT Sphere Encoder on the HIP kernels -- drop-in for the reference's models/sphere_encoder_vit.py, class SphereEncoderViT (the
paper architecture: ViT + MLP-Mixer + RoPE + sinusoidal positions): same constructor signature and defaults, state_dict keys, shapes
and order (the `pe` buffers of both positional embeddings and every block's `rotary.inv_freq` included), init RNG order, forward /
loss_function dictionaries, encode_to_vector / spherify / decode_from_sphere / sample.  Like the conv class (models/sphere_encoder.py,
whose sphere plumbing -- SphereCommon -- this shares) its perceptual term runs on VGG16 weights the caller registered
(perceptual.use_vgg16_weights) and `use_perceptual=True` raises with none registered; a non-zero `dropout` raises as well (the attention kernels have no dropout instances in their bidirectional form).

Data path, all [B, N, D] token tensors, every step a launch of libmovae_hip.so and no [N, N] matrix anywhere:
  patch embedding   a k = stride = patch convolution on the NHWC image, whose output [B, h, w, D] IS [B, N, D]; + pos (add_rows_bcast)
  transformer block LayerNorm -> qkv 1x1 conv -> attention with RoPE on the packed projection -> proj 1x1 conv -> add;
                    LayerNorm -> fc1 (bias-free) -> bias + GELU -> fc2 -> add
  mixer block       RMSNorm -> transpose -> fc(N -> T) -> bias + GELU -> fc(T -> N) -> transpose -> add; RMSNorm -> fc -> GELU -> fc -> add
  decoder tail      LayerNorm -> head 1x1 conv -> unpatchify + tanh straight into the NHWC image
The decoder's positional table rides on the final RMSNorm of mixer_dec (ops.RowNorm's `pos`).  The RoPE tables are built once per
(N, head_dim, device) on the host with the reference's expressions (ops.rope_tables)."""
import torch
import torch.nn as tnn

from .. import nn as mnn
from .. import ops
from ._base import HotPathModel, nchw_view
from .sphere_encoder import SphereCommon


class SinusoidalPosEmbedding(tnn.Module):
    """The buffer `pe` [1, max_len, dim] of the reference's module (sphere_encoder_vit.py:53-68); `table(n)`: its first n rows."""

    def __init__(self, dim, max_len=2048):
        super().__init__()
        import math

        self.dim = dim
        pe = torch.zeros(max_len, dim)
        position = torch.arange(0, max_len, dtype=torch.float32).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, dim, 2).float() * (-math.log(10000.0) / dim))
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        self.register_buffer("pe", pe.unsqueeze(0))

    def table(self, n):
        return self.pe[0, :n]

    def forward(self, x):
        return ops.add_rows_bcast(x, self.table(x.size(1)))


class RotaryEmbedding(tnn.Module):
    """The buffer `inv_freq` of the reference's module (:92-106); `tables(n, device)`: the cos / sin tables the attention kernels read."""

    def __init__(self, dim, base=10000.0, max_len=2048):
        super().__init__()
        self.dim, self.base, self.max_len = dim, base, max_len
        self.register_buffer("inv_freq", 1.0 / (base ** (torch.arange(0, dim, 2).float() / dim)))
        self._tables = {}

    def tables(self, n, device):
        """Cached per (n, device) for the current contents of `inv_freq`: an in-place change of the buffer (load_state_dict) bumps its
        version, a replaced buffer (.to(device)) has another identity; either way the tables are rebuilt."""
        if n > self.max_len:
            raise ValueError(f"RotaryEmbedding: {n} positions exceed max_len {self.max_len}")
        key = (n, device.type, device.index)
        stamp = (id(self.inv_freq), self.inv_freq._version)
        hit = self._tables.get(key)
        if hit is None or hit[0] != stamp:
            hit = self._tables[key] = (stamp, ops.rope_tables(n, self.inv_freq, device))
        return hit[1]


class PatchEmbed(tnn.Module):
    """NHWC image -> [B, N, D] (:109-122): `proj` is nn.Conv2d(C, D, patch, stride=patch)."""

    def __init__(self, img_size, patch_size, in_channels=3, embed_dim=768):
        super().__init__()
        self.img_size, self.patch_size = img_size, patch_size
        self.num_patches = (img_size // patch_size) ** 2
        self.proj = mnn.Conv2d(in_channels, embed_dim, patch_size, stride=patch_size)

    def forward(self, x_nhwc):
        y = self.proj(x_nhwc)  # [B, h, w, D]: row-major over (h, w) is the reference's flatten(2).transpose(1, 2)
        return y.reshape(y.shape[0], y.shape[1] * y.shape[2], y.shape[3])


class AttentionWithRoPE(tnn.Module):
    def __init__(self, embed_dim, num_heads, dropout=0.0):
        super().__init__()
        self.embed_dim, self.num_heads, self.head_dim = embed_dim, num_heads, embed_dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.qkv = mnn.TokenLinear(embed_dim, embed_dim * 3)
        self.proj = mnn.TokenLinear(embed_dim, embed_dim)
        self.dropout = tnn.Dropout(dropout)  # (p == 0: a placeholder that keeps the reference's module tree)
        self.rotary = RotaryEmbedding(self.head_dim)

    def forward(self, x, rope=None):
        cos, sin = rope if rope is not None else (None, None)
        return self.proj(ops.attention(self.qkv(x), self.num_heads, cos, sin))


class TransformerBlock(tnn.Module):
    def __init__(self, embed_dim, num_heads, mlp_ratio=4.0, dropout=0.0):
        super().__init__()
        self.norm1 = mnn.LayerNorm(embed_dim)
        self.attn = AttentionWithRoPE(embed_dim, num_heads, dropout)
        self.norm2 = mnn.LayerNorm(embed_dim)
        hidden = int(embed_dim * mlp_ratio)
        # (indices 1, 2 and 4 are the reference's GELU and Dropouts: parameter-free, kept for the state_dict's `mlp.0` / `mlp.3`)
        self.mlp = tnn.Sequential(mnn.TokenLinear(embed_dim, hidden), tnn.GELU(), tnn.Dropout(dropout), mnn.TokenLinear(hidden, embed_dim),
                                  tnn.Dropout(dropout))

    def forward(self, x, rope=None):
        x = ops.add(x, self.attn(self.norm1(x), rope))
        return ops.add(x, self.mlp[3](self.mlp[0](self.norm2(x), gelu=True)))


def _transpose_tokens(x):
    """[B, N, D] -> [B, D, N] (x.transpose(1, 2), materialised) through the layout kernels: N plays the image rows of a 1-wide image."""
    b, n, d = x.shape
    return ops.NhwcToNchw.apply(x.reshape(b, n, 1, d)).reshape(b, d, n)


def _transpose_back(x):
    b, d, n = x.shape
    return ops.NchwToNhwc.apply(x.reshape(b, d, n, 1)).reshape(b, n, d)


class MLPMixerBlock(tnn.Module):
    def __init__(self, num_patches, embed_dim, tokens_mlp_dim=256, channels_mlp_dim=2048):
        super().__init__()
        self.norm1 = mnn.RMSNorm(embed_dim)
        self.token_mix = tnn.Sequential(mnn.TokenLinear(num_patches, tokens_mlp_dim), tnn.GELU(), mnn.TokenLinear(tokens_mlp_dim, num_patches))
        self.norm2 = mnn.RMSNorm(embed_dim)
        self.channel_mix = tnn.Sequential(mnn.TokenLinear(embed_dim, channels_mlp_dim), tnn.GELU(), mnn.TokenLinear(channels_mlp_dim, embed_dim))

    def forward(self, x):
        t = _transpose_tokens(self.norm1(x))
        x = ops.add(x, _transpose_back(self.token_mix[2](self.token_mix[0](t, gelu=True))))
        return ops.add(x, self.channel_mix[2](self.channel_mix[0](self.norm2(x), gelu=True)))


class MLPMixer(tnn.Module):
    def __init__(self, num_patches, embed_dim, depth, tokens_mlp_dim=256, channels_mlp_dim=2048):
        super().__init__()
        self.blocks = tnn.ModuleList([MLPMixerBlock(num_patches, embed_dim, tokens_mlp_dim, channels_mlp_dim) for _ in range(depth)])
        self.norm = mnn.RMSNorm(embed_dim)

    def forward(self, x, pos=None):
        for blk in self.blocks:
            x = blk(x)
        return self.norm(x, pos)


class SphereEncoderViT(SphereCommon, HotPathModel):
    def __init__(self, img_size: int = 32, patch_size: int = 2, in_channels: int = 3, embed_dim: int = 1024, depth: int = 24,
                 num_heads: int = 16, mlp_ratio: float = 4.0, mixer_depth: int = 2, mixer_tokens_mlp_dim: int = 256,
                 mixer_channels_mlp_dim: int = 2048, latent_channels: int = 8, num_classes: int = 0, sigma_max_angle_deg: float = 80.0,
                 sigma_mix_prob: float = 0.0, sigma_mix_angle_min_deg=None, sigma_mix_angle_max_deg=None, lambda_pix_recon: float = 1.0,
                 lambda_pix_con: float = 0.5, lambda_lat_con: float = 0.1, pix_recon_smooth_l1_weight: float = 1.0,
                 pix_recon_perceptual_weight: float = 1.0, pix_con_smooth_l1_weight: float = 0.5, pix_con_perceptual_weight: float = 0.5,
                 use_perceptual: bool = True, dropout: float = 0.0, device=None):
        vgg16_weights = self._vgg16_weights_or_refuse("SphereEncoderViT", use_perceptual)
        if dropout != 0:
            raise NotImplementedError(f"SphereEncoderViT(dropout={dropout}): dropout in the attention and MLP paths is not built (the "
                                      "reference's factory never sets it; DESIGN.md section 7); pass dropout=0.0")
        super().__init__()
        if embed_dim % num_heads or (embed_dim // num_heads) % 2 or embed_dim // num_heads > 64:
            raise ValueError(f"SphereEncoderViT: head_dim = embed_dim / num_heads = {embed_dim}/{num_heads} must be an even integer <= 64 "
                             "(the RoPE attention kernels' range)")
        self.device = device
        self.img_size, self.input_size, self.patch_size, self.in_channels = img_size, img_size, patch_size, in_channels
        self.num_patches = (img_size // patch_size) ** 2
        self.num_classes = num_classes
        # the reference's construction order, which is its init RNG order
        self.patch_embed_enc = PatchEmbed(img_size, patch_size, in_channels, embed_dim)
        self.pos_embed_enc = SinusoidalPosEmbedding(embed_dim, max_len=self.num_patches)
        self.blocks_enc = tnn.ModuleList([TransformerBlock(embed_dim, num_heads, mlp_ratio, dropout) for _ in range(depth)])
        self.mixer_enc = MLPMixer(self.num_patches, embed_dim, mixer_depth, mixer_tokens_mlp_dim, mixer_channels_mlp_dim)
        self.norm_enc = mnn.RMSNorm(embed_dim)
        self.latent_proj_enc = mnn.TokenLinear(embed_dim, latent_channels)
        self.latent_proj_dec = mnn.TokenLinear(latent_channels, embed_dim)
        self.norm_dec_in = mnn.RMSNorm(embed_dim)
        self.mixer_dec = MLPMixer(self.num_patches, embed_dim, mixer_depth, mixer_tokens_mlp_dim, mixer_channels_mlp_dim)
        self.pos_embed_dec = SinusoidalPosEmbedding(embed_dim, max_len=self.num_patches)
        self.blocks_dec = tnn.ModuleList([TransformerBlock(embed_dim, num_heads, mlp_ratio, dropout) for _ in range(depth)])
        self.norm_dec_out = mnn.LayerNorm(embed_dim)
        self.head_dec = mnn.TokenLinear(embed_dim, patch_size * patch_size * in_channels)
        self._init_sphere(self.num_patches * latent_channels, sigma_max_angle_deg, sigma_mix_prob, sigma_mix_angle_min_deg,
                          sigma_mix_angle_max_deg, lambda_pix_recon, lambda_pix_con, lambda_lat_con, pix_recon_smooth_l1_weight,
                          pix_recon_perceptual_weight, pix_con_smooth_l1_weight, pix_con_perceptual_weight, vgg16_weights)

    def _rope(self, n, device, enc=True):
        """The tables of the first block's rotary module, which the reference hands to every block (:338-340)."""
        blocks = self.blocks_enc if enc else self.blocks_dec
        return blocks[0].attn.rotary.tables(n, device) if len(blocks) else None

    def prepare_for_graph(self):
        super().prepare_for_graph()
        params = list(self.parameters())
        if params and params[0].is_cuda:  # the tables exist before the capture
            self._rope(self.num_patches, params[0].device, True)
            self._rope(self.num_patches, params[0].device, False)

    def encode_to_vector(self, x):
        """Encode an image (logical NCHW) to the flat vector [B, L] (before spherify)."""
        h = self.pos_embed_enc(self.patch_embed_enc(ops.to_nhwc(x)))
        rope = self._rope(h.size(1), h.device, True)
        for blk in self.blocks_enc:
            h = blk(h, rope)
        z = self.latent_proj_enc(self.norm_enc(self.mixer_enc(h)))
        return z.reshape(z.size(0), -1)

    def decode_from_sphere(self, v):
        """Decode a spherical latent [B, L] to the image, a logical NCHW view of the NHWC buffer the last launch writes."""
        h = self.norm_dec_in(self.latent_proj_dec(v.reshape(v.size(0), self.num_patches, -1)))
        h = self.mixer_dec(h, self.pos_embed_dec.table(self.num_patches))  # (+ pos_embed_dec inside the mixer's final RMSNorm)
        rope = self._rope(h.size(1), h.device, False)
        for blk in self.blocks_dec:
            h = blk(h, rope)
        h = self.head_dec(self.norm_dec_out(h))
        return nchw_view(ops.unpatchify_act(h, self.img_size, self.img_size, self.in_channels, self.patch_size))

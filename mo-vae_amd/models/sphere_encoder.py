"""The conv Sphere Encoder on the HIP kernels -- drop-in for the reference's models/sphere_encoder.py, class SphereEncoder (same
constructor signature and defaults, state_dict keys and order, init RNG order, forward / loss_function dictionaries).  Its perceptual
term (`use_perceptual=True`, the reference's default) is perceptual.PerceptualLoss on VGG16 weights the caller has registered
(perceptual.use_vgg16_weights, or $MOVAE_VGG16_WEIGHTS): this build fetches none, so with nothing registered
`use_perceptual=True` raises.

The latent is RMS-normalised onto the sphere of radius sqrt(L); there is no KL term.  One step makes two encoder and two decoder
passes: v = spherify(E(x)); a jitter angle per image gives sigma = tan(angle) and sigma_sub = s * sigma; recons = D(spherify(v +
sigma_sub e)), x_recon_NOISY = D(spherify(v + sigma e)); v_enc_dec = spherify(E(x_recon_NOISY)).  The three objectives
(pix_recon, pix_con, lat_con) each reach every parameter, so the Jacobian spans them all (`features is None`), as for
models/recursive_vaes.py, whose plumbing this reuses: every encoder / decoder call runs BatchNorm in training mode (two updates of
the running statistics per module per step, as in the reference), the decoder's output-activation link stays unused (recons and
x_recon_NOISY have two readers each), and train pulls the Jacobian rows back from the loss op (autojac.backward_through).

Everything between encoder_proj and the decoder calls is one launch (ops.SphereLatents), the loss_function two (ops.SphereLosses); with
the perceptual term the three images are normalised in two launches, each goes through the VGG stack once (the features of `recons`
serve as the prediction of pix_recon and, detached, as the target of pix_con), and one ops.CombineLosses launch forms the four values.
The noise: eager mode draws with torch in the reference's order (rand, [rand, rand], rand, randn); `noise_override` = {"u": [B, 4],
"e": [B, L]} replaces the draws (parity tests; u's columns are the angle, mix-mask, mix-angle and s uniforms); after
prepare_for_graph the draws are made inside the SphereLatents launch.  Eval mode draws noise too, like the reference."""
import contextlib
import math
from math import sqrt

import torch

from .. import nn as mnn
from .. import ops
from .. import perceptual
from ._base import nchw_view
from .vae import VAE


class SphereCommon:
    """What the conv and the ViT Sphere Encoder share (mixed in ahead of a HotPathModel): the hyperparameters, the noise schedule and
    its draws, spherify, forward, loss_function and sample.  The class supplies encode_to_vector(x) -> [B, L] and
    decode_from_sphere(v) -> a logical NCHW view of an NHWC buffer."""
    graph_safe = True
    #: internal: every loss is an output of ops.SphereLosses, so train can pull the K Jacobian rows back from its inputs.  With the
    #: perceptual term the losses come out of ops.CombineLosses, which has no `input_cotangents`: autojac.backward_through then takes
    #: one autograd pass per loss, its fallback
    _jacobian_from_loss_op = True
    #: {"u": [B, 4], "e": [B, L]} to replace the draws of forward (parity tests)
    noise_override = None

    @staticmethod
    def _vgg16_weights_or_refuse(name, use_perceptual):
        """The registered VGG16 weights for use_perceptual=True (None otherwise); nothing registered: the refusal."""
        weights = perceptual.registered_vgg16_weights() if use_perceptual else None
        if use_perceptual and weights is None:
            raise NotImplementedError(f"{name}(use_perceptual=True) needs the pretrained VGG16 weights of the reference's "
                                      "PerceptualLoss, which this build does not carry (DESIGN.md section 7); register yours with "
                                      f"movae_amd.perceptual.use_vgg16_weights(path) or ${perceptual.ENV_VAR}, or pass use_perceptual=False")
        return weights

    def _init_sphere(self, L, sigma_max_angle_deg, sigma_mix_prob, sigma_mix_angle_min_deg, sigma_mix_angle_max_deg, lambda_pix_recon,
                     lambda_pix_con, lambda_lat_con, pix_recon_smooth_l1_weight, pix_recon_perceptual_weight, pix_con_smooth_l1_weight,
                     pix_con_perceptual_weight, vgg16_weights=None):
        self.L = L
        self.radius = sqrt(L)
        self.sigma_max_angle_deg = float(sigma_max_angle_deg)
        self.sigma_max = math.tan(math.radians(self.sigma_max_angle_deg))
        self.sigma_mix_prob = float(sigma_mix_prob)
        self.sigma_mix_angle_min_deg = float(sigma_mix_angle_min_deg) if sigma_mix_angle_min_deg is not None else None
        self.sigma_mix_angle_max_deg = float(sigma_mix_angle_max_deg) if sigma_mix_angle_max_deg is not None else None
        self.lambda_pix_recon, self.lambda_pix_con, self.lambda_lat_con = lambda_pix_recon, lambda_pix_con, lambda_lat_con
        self.pix_recon_smooth_l1_weight, self.pix_recon_perceptual_weight = pix_recon_smooth_l1_weight, pix_recon_perceptual_weight
        self.pix_con_smooth_l1_weight, self.pix_con_perceptual_weight = pix_con_smooth_l1_weight, pix_con_perceptual_weight
        # models/sphere_encoder.py:126-130: the last submodule registered, so its keys close the state_dict
        self.use_perceptual = vgg16_weights is not None
        self.perceptual_loss = perceptual.PerceptualLoss(vgg16_weights) if self.use_perceptual else None
        # objectives for MTL / logging (models/sphere_encoder.py:133-137: placeholders; loss_function computes the terms)
        zero = lambda *_: torch.tensor(0.0, device=next(self.parameters()).device)  # noqa: E731
        self.objectives = {"pix_recon": zero, "pix_con": zero, "lat_con": zero}
        self.features = None  # every objective reaches every parameter

    # -- the noise schedule ------------------------------------------------------------------------------------------------------
    def _mix_enabled(self):
        lo, hi = self.sigma_mix_angle_min_deg, self.sigma_mix_angle_max_deg
        return self.sigma_mix_prob > 0 and lo is not None and hi is not None and hi > lo

    def _schedule(self):
        """(angle_max_deg, mix_prob or 0, mix_min_deg, mix_max_deg) of ops.SphereLatents"""
        if self._mix_enabled():
            return (self.sigma_max_angle_deg, self.sigma_mix_prob, self.sigma_mix_angle_min_deg, self.sigma_mix_angle_max_deg)
        return (self.sigma_max_angle_deg, 0.0, 0.0, 0.0)

    def _draws(self, batch, device, dtype):
        """(u [B, 4], e [B, L]) from noise_override or from torch in the reference's order (models/sphere_encoder.py:203-218)."""
        if self.noise_override is not None:
            return tuple(self.noise_override[k].to(device=device, dtype=dtype) for k in ("u", "e"))
        zero = torch.zeros(batch, 1, device=device, dtype=dtype)
        angle = torch.rand(batch, 1, device=device, dtype=dtype)
        mask, mix = (torch.rand(batch, 1, device=device), torch.rand(batch, 1, device=device, dtype=dtype)) if self._mix_enabled() else (zero, zero)
        s = torch.rand(batch, 1, device=device, dtype=dtype)
        e = torch.randn(batch, self.L, device=device, dtype=dtype)
        return torch.cat([angle, mask.to(dtype), mix, s], dim=1), e

    # -- reference API -----------------------------------------------------------------------------------------------------------
    def spherify(self, z, add_noise=False, sigma=None, e=None):
        """Project z onto the sphere; with add_noise, sigma and e: spherify(spherify(z) + sigma * e) (the noise is added to the
        already-spherified v, models/sphere_encoder.py:146-162).  sigma: a number, or a tensor of 1 or B values."""
        if add_noise and sigma is not None and e is not None:
            return ops.spherify(z, self.radius, sigma, e)
        return ops.spherify(z, self.radius)

    def forward(self, x):
        z = self.encode_to_vector(x)
        if self.noise_override is None and self.noise_on_device and z.is_cuda:
            lat = ops.sphere_latents(z, self._schedule(), self.radius, state=self._noise_state(z.device))
        else:
            u, e = self._draws(x.size(0), z.device, z.dtype)
            lat = ops.sphere_latents(z, self._schedule(), self.radius, e=e, u=u)
        v, v_noisy, v_noisy_small, sigma, sigma_sub = lat[:5]
        recons = self.decode_from_sphere(v_noisy_small)
        x_recon_noisy = self.decode_from_sphere(v_noisy)
        v_enc_dec = self.spherify(self.encode_to_vector(x_recon_noisy))  # (reuses x_recon_NOISY: no third decoder pass)
        return {"recons": recons, "v": v, "v_noisy": v_noisy, "v_noisy_small": v_noisy_small, "x_recon_NOISY": x_recon_noisy,
                "x_recon_noisy_small_sg": recons.detach(), "v_enc_dec": v_enc_dec, "sigma": sigma, "sigma_sub": sigma_sub}

    def loss_function(self, inputs, args: dict) -> dict:
        sg = ops.to_nhwc(args["x_recon_noisy_small_sg"].detach())
        r, x, xn = ops.to_nhwc(args["recons"]), ops.to_nhwc(inputs), ops.to_nhwc(args["x_recon_NOISY"])
        lam = (self.lambda_pix_recon, self.lambda_pix_con, self.lambda_lat_con)
        w_sl1 = (self.pix_recon_smooth_l1_weight, self.pix_con_smooth_l1_weight)
        names = ("pix_recon", "pix_con", "lat_con", "total_loss")
        w_rec, w_con = self.pix_recon_perceptual_weight, self.pix_con_perceptual_weight
        pl = self.perceptual_loss if self.use_perceptual else None
        if pl is None or (w_rec <= 0 and w_con <= 0):  # (_pixel_loss, models/sphere_encoder.py:243-247: the term needs a positive weight)
            return dict(zip(names, ops.sphere_losses(r, x, xn, args["v"], args["v_enc_dec"], lam, w_sl1, sg=sg)))
        # pix = lambda * (w_sl1 * smooth_l1 + w_perc * perceptual): the unweighted sums' terms, then one launch for the four values
        sl1_rec, sl1_con, lat, _ = ops.sphere_losses(r, x, xn, args["v"], args["v_enc_dec"], (1.0, 1.0, 1.0), w_sl1, sg=sg)
        images = [r] + ([x] if w_rec > 0 else []) + ([xn] if w_con > 0 else [])
        normed = list(ops.vgg_prep(*images))
        # the features of recons: the prediction of pix_recon and, detached, the target of pix_con (the reference computes them twice)
        with contextlib.nullcontext() if w_rec > 0 else torch.no_grad():
            f_r = pl.features(normed.pop(0))
        terms, rows = [sl1_rec, sl1_con, lat], [[lam[0], 0.0, 0.0], [0.0, lam[1], 0.0], [0.0, 0.0, lam[2]]]
        if w_rec > 0:
            with torch.no_grad():
                f_x = pl.features(normed.pop(0))
            terms.append(pl.feature_mse(f_r, f_x, w_rec))
            rows = [row + [lam[0] if k == 0 else 0.0] for k, row in enumerate(rows)]
        if w_con > 0:
            terms.append(pl.feature_mse(pl.features(normed.pop(0)), f_r, w_con))
            rows = [row + [lam[1] if k == 1 else 0.0] for k, row in enumerate(rows)]
        return dict(zip(names, ops.combine_losses(terms, rows)))

    def sample(self, num_samples=1, device=None, steps=1, share_noise=True):
        """One-step generation x = D(spherify(e)), e ~ N(0, I); steps > 1 iterates encode / decode at the fixed noise strength
        sigma_max, with the same e in every step when share_noise (models/sphere_encoder.py:285-308)."""
        if device is None:
            device = next(self.parameters()).device
        self.eval()
        with torch.no_grad():
            e = torch.randn(num_samples, self.L, device=device)
            x = self.decode_from_sphere(self.spherify(e))
            for _ in range(steps - 1):
                z = self.encode_to_vector(x)
                e_step = e if share_noise else torch.randn(num_samples, self.L, device=device)
                x = self.decode_from_sphere(self.spherify(z, add_noise=True, sigma=self.sigma_max, e=e_step))
        return x


class SphereEncoder(SphereCommon, VAE):
    def __init__(self, latent_dim: int = 2048, sigma_max_angle_deg: float = 80.0, sigma_mix_prob: float = 0.0,
                 sigma_mix_angle_min_deg=None, sigma_mix_angle_max_deg=None, lambda_pix_recon: float = 1.0, lambda_pix_con: float = 0.5,
                 lambda_lat_con: float = 0.1, pix_recon_smooth_l1_weight: float = 1.0, pix_recon_perceptual_weight: float = 1.0,
                 pix_con_smooth_l1_weight: float = 0.5, pix_con_perceptual_weight: float = 0.5, use_perceptual: bool = True, **kwargs):
        vgg16_weights = self._vgg16_weights_or_refuse("SphereEncoder", use_perceptual)
        super().__init__(latent_dim=latent_dim, **kwargs)
        # models/sphere_encoder.py:102-107: the VAE's heads go, decoder_input is replaced in place, encoder_proj is registered last;
        # the RNG draws follow the VAE's: encoder_proj, then the new decoder_input
        feat = self.hidden_dims[-1] * (self.input_size // (2 ** len(self.hidden_dims))) ** 2
        del self.mu
        del self.log_var
        self.encoder_proj = mnn.Linear(feat, latent_dim)
        self.decoder_input = mnn.Linear(latent_dim, feat)

        self._init_sphere(latent_dim, sigma_max_angle_deg, sigma_mix_prob, sigma_mix_angle_min_deg, sigma_mix_angle_max_deg, lambda_pix_recon,
                          lambda_pix_con, lambda_lat_con, pix_recon_smooth_l1_weight, pix_recon_perceptual_weight, pix_con_smooth_l1_weight,
                          pix_con_perceptual_weight, vgg16_weights)

    def encode_to_vector(self, x):
        """Encode to the flat vector (before spherify)."""
        return self.encoder_proj(self.encoder(ops.to_nhwc(x)))

    def decode_from_sphere(self, v):
        y = self.final_layer(self.decoder(self.decoder_input(v)))
        self.final_layer._out_link = None  # the output activation's link stays unused (see the module docstring)
        self._recons_link = None
        return nchw_view(y)

    def encode(self, x):
        """(v,) on the sphere, for compatibility; no mu / log_var."""
        return (self.spherify(self.encode_to_vector(x)),)

    def reparameterize(self, mu, log_var):
        return mu

    def decode(self, z):
        """Decode a latent: taken as it is when it lies on the sphere (norm within 1e-2 of the radius), else spherified first."""
        if z.dim() == 1:
            z = z.unsqueeze(0)
        norm = z.norm(dim=-1, keepdim=True)
        if not torch.allclose(norm, torch.full_like(norm, self.radius), atol=1e-2):
            z = self.spherify(z)
        return self.decode_from_sphere(z)

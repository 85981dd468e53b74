"""The reference's multi-objective VAEs on the HIP kernels -- drop-ins for models/recursive_kl_vae.py, models/cycle_vae.py and
models/recursive_cyclic_vae.py (same constructor signatures, state_dict keys, forward / loss_function dictionaries, weight quirks).

They reuse the VAE's encoder and decoder several times per step: RecursiveKL encodes the reconstruction again (mu_hat, log_var_hat),
Cycle decodes a prior sample and encodes the result (mu_gen), RC-VAE does both.  Every call runs BatchNorm in training mode and
updates its running statistics, as in the reference (three encoder and two decoder updates per RC-VAE step).

What the fusion machinery assumes about one call per module per step, and why it holds here:
  * the decoder's output activation link (VAE._recons_link) is left unused: `recons` has two readers (the reconstruction loss and
    the second encoder pass), so the loss kernel differentiates through tanh / sigmoid like any other reader and the producing conv
    runs its own activation backward (ops._act_take finds no `applied` tensor);
  * the ActLinks / LazyBNs inside nn.Stack live per call (each encoder / decoder call builds its own), the encoder ends in a
    flatten (a LazyBN never leaves it), and `x_gen` enters the encoder unlinked;
  * the Jacobian spans all parameters (`features is None`): by default one torch.autograd pass per loss (the engine sums a reused
    parameter's uses; no gradient sink, in-place accumulation or parked reduce is armed).  MOVAE_BATCHED_FULL_JACOBIAN=1 pulls the K cotangents of the loss kernel's inputs back together instead
    (autojac.backward_through): the Jacobian-row sinks are consumed by a parameter's first use and the walker adds the later uses
    before the leaf copy.

All loss terms, their weights, the recursive-KL annealing and the total come from one fused kernel pair (ops.RecursiveLosses).  In
graph mode (prepare_for_graph) z_prior is drawn in the reparameterisation launch (ops.ReparameterizePriorRNG) and the annealing
counter lives on the device; eager mode draws z_prior with torch.randn like the reference."""
import torch

from .. import objectives as O
from .. import ops
from .vae import VAE


def _cycle_loss(z_prior, mu_gen):
    """models/cycle_vae.py:17-19 (stand-alone objective; loss_function computes the term inside ops.RecursiveLosses)."""
    return ((z_prior - mu_gen) ** 2).sum(dim=1).mean()


class _MultiPassVAE(VAE):
    """Shared forward / loss plumbing; subclasses set the two switches and own their class-level step counter."""

    _recursive_kl = False
    _cycle = False
    graph_safe = True
    #: device copy of the annealing counter (graph mode: prepare_for_graph), advanced inside the loss kernel
    _iter_dev = None
    #: set to a tensor to replace the prior draw z_prior (parity tests; see eps_override)
    z_prior_override = None

    #: internal: every loss is an output of the loss kernel (ops.RecursiveLosses), so train can pull the K Jacobian rows back from
    #: its inputs (autojac.backward_through); `features is None` stays the public protocol
    _jacobian_from_loss_op = True

    def _tick(self):
        """Advance the class-level step counter on the host and return min(num_iter / anneal_steps, 1)."""
        raise NotImplementedError

    def _counter(self):
        raise NotImplementedError

    def prepare_for_graph(self):
        super().prepare_for_graph()
        if self._recursive_kl and self._iter_dev is None:
            self._iter_dev = torch.tensor(float(self._counter()), dtype=torch.float32, device=next(self.parameters()).device)

    def _latent_and_prior(self, mu, log_var, batch):
        """(z, z_prior): one device launch for both in graph mode, else the reference's draws in its order (randn_like, then randn)."""
        fused = (self._cycle and self.noise_on_device and mu.is_cuda and self.eps_override is None and self.z_prior_override is None)
        if fused:
            return ops.reparameterize_prior_rng(mu, log_var, self._noise_state(mu.device), batch)
        z = self.reparameterize(mu, log_var)
        if not self._cycle:
            return z, None
        if self.z_prior_override is not None:
            return z, self.z_prior_override.to(device=mu.device, dtype=mu.dtype)
        return z, torch.randn(batch, self.latent_dim, device=mu.device)

    def forward(self, x):
        mu, log_var = self.encode(x)
        z, z_prior = self._latent_and_prior(mu, log_var, x.size(0))
        recons = self.decode(z)
        self._recons_link = None  # recons has a second reader (see the module docstring)
        out = {"recons": recons, "mu": mu, "log_var": log_var, "z": z}
        if self._recursive_kl:
            out["mu_hat"], out["log_var_hat"] = self.encode(recons)
        if self._cycle:
            x_gen = self.decode(z_prior)
            self._recons_link = None
            mu_gen, log_var_gen = self.encode(x_gen)
            out.update(z_prior=z_prior, x_gen=x_gen, mu_gen=mu_gen, log_var_gen=log_var_gen)
        return out

    def _anneal(self):
        if not self.training:
            return (None, 1.0, 1.0, False)
        if self._iter_dev is not None:
            return (self._iter_dev, 0.0, float(self.anneal_steps), True)
        return (None, self._tick(), float(self.anneal_steps), True)

    def loss_function(self, inputs, args: dict) -> dict:
        lw = self.lambda_weights
        rec_fn = self.objectives["reconstruction_loss"]
        x, r = ops.to_nhwc(inputs), ops.to_nhwc(args["recons"])
        kw = {}
        if self._recursive_kl:
            kw.update(mu_hat=args["mu_hat"], log_var_hat=args["log_var_hat"], w_kl=lw["recursive_kld_loss"], anneal=self._anneal())
        if self._cycle:
            kw.update(z_prior=args["z_prior"], mu_gen=args["mu_gen"], w_cyc=lw["cycle_loss"])
        vals = ops.recursive_losses(r, x, rec_fn.kind, lw["reconstruction_loss"], **kw)
        keys = ["reconstruction_loss"] + (["recursive_kld_loss"] if self._recursive_kl else []) + (["cycle_loss"] if self._cycle else [])
        return dict(zip(keys + ["total_loss"], vals))


def _resolve_weights(given, form):
    """The loss-weight forms of one architecture, from its table entry `form` = (unset, long, base_of, added):
      unset    what an absent `lambda_weights` argument stands for (a list);
      long     a list of at least this many numbers is the model's own form: the VAE base receives base_of(list) and every added
               term takes list[index] (its `added` entry (index, fallback)) when the list is long enough, else its fallback;
      any other form (a shorter list, a dict, None) reaches the VAE base unchanged -- which validates it -- and the added terms
      take their fallbacks.  A fallback is a number, or the name of a base weight that the term replaces (removed in every form; its value
      is the fallback).
    -> (what the VAE base receives, {added term: index or None}, long form?)"""
    unset, long, base_of, added = form
    given = unset if given is _UNSET else given
    is_long = isinstance(given, list) and len(given) >= long
    picks = {k: (i if is_long and i < len(given) else None) for k, (i, _) in added.items()}
    return (base_of(given) if is_long else given), picks, given


_UNSET = object()


def _apply_added_weights(model, given, picks, added):
    """Objectives / weights of the added terms, appended after the VAE's, in table order."""
    for k, i in picks.items():
        fallback = added[k][1]
        if isinstance(fallback, str):  # the term replaces that base weight, which goes in any case
            fallback = model.lambda_weights.pop(fallback)
        w = given[i] if i is not None else fallback
        model.lambda_weights[k] = w


#: per architecture: (unset, long, base_of, {added term: (list index, fallback)}), see _resolve_weights -- models/recursive_kl_vae.py:42-60,
#: cycle_vae.py:27-41, recursive_cyclic_vae.py:108-130
_WEIGHT_FORMS = {
    "RecursiveKLVAE": ([1.0, 0.00025], 2, lambda w: w[:2], {"recursive_kld_loss": (2, "kld_loss")}),
    "CycleVAE": ([1.0, 0.00025], 2, lambda w: [w[0], 0.0], {"cycle_loss": (1, 0.00025)}),
    "RecursiveCyclicVAE": ([1.0, 0.00025, 0.00025], 3, lambda w: [w[0], 0.0],
                           {"recursive_kld_loss": (1, 0.00025), "cycle_loss": (2, 0.00025)}),
}


class _WeightedMultiPassVAE(_MultiPassVAE):
    def _build(self, kwargs, added_objectives, anneal_steps=None):
        form = _WEIGHT_FORMS[type(self).__name__]
        base, picks, given = _resolve_weights(kwargs.pop("lambda_weights", _UNSET), form)
        super().__init__(lambda_weights=base, **kwargs)
        self.features = None  # every objective reaches every parameter: the Jacobian spans them all
        if anneal_steps is not None:
            self.anneal_steps = anneal_steps
        for k, fn in added_objectives.items():
            if isinstance(fn, str):  # an objective of the VAE's taken over under a new name
                fn = self.objectives.pop(fn)
            self.objectives[k] = fn
        _apply_added_weights(self, given, picks, form[3])


class RecursiveKLVAE(_WeightedMultiPassVAE):
    """models/recursive_kl_vae.py: KL on the re-encoded reconstruction, linearly annealed over recursive_kld_anneal_steps."""

    num_iter = 0  # class-level step counter shared by all instances (models/recursive_kl_vae.py:49)
    _recursive_kl = True

    def __init__(self, recursive_kld_anneal_steps: int = 25000, **kwargs):
        self._build(kwargs, {"recursive_kld_loss": "kld_loss"}, recursive_kld_anneal_steps)

    def _tick(self):
        RecursiveKLVAE.num_iter += 1
        return min(RecursiveKLVAE.num_iter / self.anneal_steps, 1.0)

    def _counter(self):
        return RecursiveKLVAE.num_iter


class CycleVAE(_WeightedMultiPassVAE):
    """models/cycle_vae.py: reconstruction plus latent cycle consistency ||z_prior - enc_mean(dec(z_prior))||^2 (kld_loss stays
    among the objectives with weight 0 in the list form, and never appears in the loss dict)."""

    _cycle = True

    def __init__(self, **kwargs):
        self._build(kwargs, {"cycle_loss": _cycle_loss})


class RecursiveCyclicVAE(_WeightedMultiPassVAE):
    """models/recursive_cyclic_vae.py (RC-VAE): reconstruction, annealed recursive KL and latent cycle consistency; every
    objective reaches both the encoder and the decoder (a dense K x m Jacobian)."""

    num_iter = 0  # models/recursive_cyclic_vae.py:117, separate from RecursiveKLVAE's
    _recursive_kl = True
    _cycle = True

    def __init__(self, recursive_kld_anneal_steps: int = 25000, **kwargs):
        self._build(kwargs, {"recursive_kld_loss": O.kl_divergence, "cycle_loss": _cycle_loss}, recursive_kld_anneal_steps)

    def _tick(self):
        RecursiveCyclicVAE.num_iter += 1
        return min(RecursiveCyclicVAE.num_iter / self.anneal_steps, 1.0)

    def _counter(self):
        return RecursiveCyclicVAE.num_iter

#!/usr/bin/env python3
"""Golden vectors of the recursive-KL / cycle / recursive-cyclic VAEs (runs ONLY in the build container, never on the GPU box).

Imports the reference's models/__init__.py (get_network) by path, with the placeholder modules of generate_golden.py for its
absent third-party imports, and records for one tiny network per architecture (two for RC-VAE): the initial state_dict, the
input, the recorded noise draws (eps of randn_like, z_prior of randn), every forward output, the loss dict, the per-loss gradients
of every parameter by plain autograd (the Jacobian rows), the summed gradient, the state after one Adam step, a second step's
losses (the annealing counter) and an eval-mode reconstruction.  recursive_vaes_quirks.npz holds the factory's weight table:
which loss_weights forms build which weights and which raise.

Usage:  python tests/golden/generate_recursive_vaes.py        (seconds)
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("MOVAE_REFERENCE", "/root/reference")

#: (tag, arch, seed, B, input_size, latent_dim, hidden_dims, loss_weights, recursive_kld_anneal_steps, objective)
CASES = [
    ("recursive_kl_vae_tiny", "recursive_kl_vae", 42, 4, 16, 6, [8, 16], [1.0, 0.05], 3, "mse"),
    ("cycle_vae_tiny", "cycle_vae", 7, 4, 16, 6, [8, 16], [1.0, 0.05], 3, "mse"),
    ("rc_vae_tiny", "rc_vae", 11, 4, 16, 6, [8, 16], [1.0, 0.05, 0.02], 3, "mse"),
    ("rc_vae_tiny_bce", "recursive_cyclic_vae", 5, 3, 16, 4, [4, 8], [0.5, 0.1, 0.03], 2, "bce"),
]

#: (arch, loss_weights) of the factory table; dataset_size 1000, batch_size 4
QUIRKS = [
    ("recursive_kl_vae", None), ("recursive_kl_vae", [0.7, 0.3]), ("recursive_kl_vae", [0.7, 0.3, 0.2]), ("recursive_kl_vae", [0.7]),
    ("recursive_kl_vae", {"reconstruction_loss": 1.0, "kld_loss": 0.5}),
    ("cycle_vae", None), ("cycle_vae", [0.7, 0.3]), ("cycle_vae", [0.7, 0.3, 0.2]), ("cycle_vae", [0.7]),
    ("cycle_vae", {"reconstruction_loss": 1.0, "kld_loss": 0.5}), ("cycle_vae", {"reconstruction_loss": 1.0, "cycle_loss": 0.5}),
    ("rc_vae", None), ("rc_vae", [0.7, 0.3, 0.2]), ("rc_vae", [0.7, 0.3]), ("rc_vae", [0.7, 0.3, 0.2, 0.1]), ("rc_vae", [0.7]),
    ("rc_vae", {"reconstruction_loss": 1.0, "kld_loss": 0.5}),
    ("recursive_cyclic_vae", [0.9, 0.1, 0.01]),
]


def _gg():
    spec = importlib.util.spec_from_file_location("_generate_golden", os.path.join(HERE, "generate_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _CaptureRandn:
    """Records every torch.randn draw (the cycle branch's z_prior) made inside the block; with `replay` returns those instead."""

    def __init__(self, replay=None):
        self.draws, self.replay = [], None if replay is None else iter(replay)
        self._orig = torch.randn

    def __enter__(self):
        def wrapped(*a, **k):
            if self.replay is not None:
                return next(self.replay).clone()
            e = self._orig(*a, **k)
            self.draws.append(e.clone())
            return e

        torch.randn = wrapped
        return self

    def __exit__(self, *exc):
        torch.randn = self._orig


def _reset_counters():
    from models.recursive_cyclic_vae import RecursiveCyclicVAE
    from models.recursive_kl_vae import RecursiveKLVAE

    RecursiveKLVAE.num_iter = 0
    RecursiveCyclicVAE.num_iter = 0


def model_fixture(gg, tag, arch, seed, B, size, latent, hidden, lw, steps, objective):
    from models import get_network

    _np = gg._np
    out = {}
    args = gg._Args(arch=arch, batch_size=B, dataset_size=1000, recons_objective=objective, recons_activation=None, loss_weights=list(lw),
                    latent_dim=latent, hidden_dims=list(hidden), recursive_kld_anneal_steps=steps)
    torch.manual_seed(seed)
    np.random.seed(seed)
    _reset_counters()
    net = get_network(size, num_channels=3, args=args, device=torch.device("cpu"))
    net.train()
    for k, v in net.state_dict().items():
        out[f"sd0.{k}"] = _np(v)
    x = torch.rand(B, 3, size, size, generator=torch.Generator().manual_seed(seed + 1))
    out["x"] = _np(x)
    out["meta"] = np.array([f"arch={arch}", f"seed={seed}", f"B={B}", f"input_size={size}", f"objective={objective}", "dataset_size=1000",
                            f"latent_dim={latent}", f"hidden_dims={hidden}", f"recursive_kld_anneal_steps={steps}"])
    out["loss_weights"] = np.array(lw, dtype=np.float64)
    out["lambda_weights"] = np.array([f"{k}={v!r}" for k, v in net.lambda_weights.items()])
    out["objectives"] = np.array(list(net.objectives.keys()))
    with gg._Capture() as cap, _CaptureRandn() as capr:
        outputs = net(x)
    assert len(cap.draws) == 1 and len(capr.draws) == (0 if arch == "recursive_kl_vae" else 1)
    out["eps"] = _np(cap.draws[0])
    if capr.draws:
        out["z_prior"] = _np(capr.draws[0])
    loss_dict = net.loss_function(x, args=outputs)
    for k, v in outputs.items():
        out[f"out.{k}"] = _np(v)
    for k, v in loss_dict.items():
        out[f"loss.{k}"] = _np(v)
    names = [n for n, _ in net.named_parameters()]
    params = [p for _, p in net.named_parameters()]
    comp = [(k, v) for k, v in loss_dict.items() if k != "total_loss"]
    for i, (k, v) in enumerate(comp):
        gs = torch.autograd.grad(v, params, retain_graph=True, allow_unused=True)
        for n, p, g in zip(names, params, gs):
            out[f"gloss.{i}.{n}"] = _np(g if g is not None else torch.zeros_like(p))
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    opt.zero_grad()
    loss_dict["total_loss"].backward()
    for n, p in zip(names, params):
        out[f"gsum.{n}"] = _np(p.grad if p.grad is not None else torch.zeros_like(p))
    opt.step()
    for k, v in net.state_dict().items():
        out[f"sd1.{k}"] = _np(v)
    with gg._Replay(cap.draws), _CaptureRandn(capr.draws):
        outputs2 = net(x)
    for k, v in net.loss_function(x, args=outputs2).items():
        out[f"loss2.{k}"] = _np(v)
    net.eval()
    with torch.no_grad(), gg._Replay(cap.draws), _CaptureRandn(capr.draws):
        oe = net(x)
        le = net.loss_function(x, args=oe)
    out["eval.recons"] = _np(oe["recons"])
    for k, v in le.items():
        out[f"eval_loss.{k}"] = _np(v)
    path = os.path.join(HERE, f"{tag}.npz")
    np.savez_compressed(path, **out)
    print(f"{tag}.npz keys={len(out)} bytes={os.path.getsize(path)}")


def quirks_fixture(gg):
    from models import get_network

    cases, results = [], []
    for arch, lw in QUIRKS:
        args = gg._Args(arch=arch, batch_size=4, dataset_size=1000, recons_objective="mse", recons_activation=None,
                        loss_weights=None if lw is None else (dict(lw) if isinstance(lw, dict) else list(lw)), latent_dim=4,
                        hidden_dims=[4, 8], recursive_kld_anneal_steps=10)
        try:
            net = get_network(16, num_channels=3, args=args, device=torch.device("cpu"))
            res = repr({"objectives": list(net.objectives.keys()), "lambda_weights": dict(net.lambda_weights),
                        "features": net.features, "anneal_steps": getattr(net, "anneal_steps", None)})
        except Exception as e:  # noqa: BLE001 -- the table records the exception type
            res = f"raises {type(e).__name__}"
        cases.append(repr((arch, lw)))
        results.append(res)
        print(arch, lw, "->", res)
    path = os.path.join(HERE, "recursive_vaes_quirks.npz")
    np.savez_compressed(path, case=np.array(cases), result=np.array(results))


if __name__ == "__main__":
    gg = _gg()
    gg._install_placeholders()
    sys.path.insert(0, REF)
    torch.set_num_threads(8)
    for c in CASES:
        model_fixture(gg, *c)
    quirks_fixture(gg)

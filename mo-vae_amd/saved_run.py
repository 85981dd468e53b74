"""The three tools that use a saved run (the repository's evaluate.py, train_prior.py and generate_samples.py are their command
lines): score it again (reference evaluate.py), train a prior on its autoencoder (train_prior_vqvae*.py) and draw pictures from it
(generate_samples_pixelcnn_vqvae*.py).  Each `*_main(argv)` returns what it printed or wrote."""
import math
import os
import types
from argparse import ArgumentParser

import torch

from . import _lib as L
from . import checkpoint, visual
from . import prior as _prior
from . import train
from .metrics import NAN_RESULT, build_hv_indicator

_DEVICE = "cuda:0" if torch.cuda.is_available() else "cpu"
_SAMPLERS = sorted(_prior.PRIOR_SAMPLERS)


def _device(name):
    device = torch.device(name)
    if device.type != "cuda":
        raise RuntimeError("the MI355X hot path needs a HIP device (--device cuda:N); there is no CPU path")
    torch.cuda.set_device(device)
    return device


def _with(run_args, **over):
    """The run's namespace with the given entries replaced (None keeps the run's value)."""
    return types.SimpleNamespace(**{**vars(run_args), **{k: v for k, v in over.items() if v is not None}})


def _dataset(run_args, name, data_dir):
    return train.get_dataset(name or run_args.dataset, data_dir=data_dir or getattr(run_args, "data_dir", "./data"),
                             normalize=getattr(run_args, "normalize_inputs", False), max_items=getattr(run_args, "max_items", None))


# ---- evaluate.py ----------------------------------------------------------------------------------------------------------------------
def evaluate_parser():
    p = ArgumentParser(description="Evaluate a saved run on its test set")
    p.add_argument("--arch", type=str, required=True)
    p.add_argument("--dataset", type=str, required=True)
    p.add_argument("--model_path", type=str, required=True)
    p.add_argument("--device", type=str, default=_DEVICE)
    p.add_argument("--batch_size", type=int, default=128)
    p.add_argument("--num_workers", type=int, default=0)
    p.add_argument("--max_fid_samples", type=int, default=5000)
    p.add_argument("--max_gen_metrics_samples", type=int, default=5000)
    p.add_argument("--seed", type=int, default=None)
    # additions of this build
    p.add_argument("--data_dir", type=str, default=None, help="where the dataset's files are (default: the run's --data_dir)")
    p.add_argument("--prior_path", type=str, default=None,
                   help="a prior checkpoint or the run directory that holds one: VQ architectures then sample through it")
    p.add_argument("--prior_sampler", type=str, default="full", choices=_SAMPLERS)
    p.add_argument("--pixelcnn_temperature", type=float, default=1.0)
    p.add_argument("--gen_metrics", choices=["off", "on"], default="on")
    p.add_argument("--gen_precision_recall", action="store_true")
    return p


def _fmt(value, name):
    if value is None or (isinstance(value, float) and math.isnan(value)):
        return "N/A"
    if name in ("psnr", "ssnr"):
        return f"{value:.2f} dB"
    if name == "hv":
        return f"{value:.6e}"
    if "codebook_usage" in name:
        return f"{value:.2f}%"
    if name in ("ssim", "lpips", "rfid", *train.GEN_METRIC_KEYS):
        return f"{value:.4f}"
    return f"{value:.6e}" if (abs(value) < 1e-3 or abs(value) > 1e3) else f"{value:.6f}"  # a loss


def _table(title, rows):
    width = max(len(n) for n, _ in rows) + 5
    print("\n" + "=" * 80 + f"\n{title}\n" + "=" * 80)
    print(f"{'Metric':<{width}} {'Value':>20}\n" + "-" * (width + 21))
    for n, v in rows:
        print(f"{n:<{width}} {v:>20}")


def print_results_table(losses, recon, gen, hv):
    """evaluate.py:109-207: the three tables (losses with the hypervolume, reconstruction metrics, generative metrics)."""
    rows = [(k, _fmt(v, k)) for k, v in losses.items()]
    if hv is not None:
        rows.append(("Hypervolume (HV)", _fmt(hv, "hv")))
    _table("TEST LOSSES (Training Objectives)", rows)
    _table("RECONSTRUCTION METRICS", [(n, _fmt(recon.get(k, float("nan")), k)) for n, k in
                                      (("rFID", "rfid"), ("PSNR", "psnr"), ("SSIM", "ssim"), ("LPIPS", "lpips"))])
    names = [("gFID", "gfid"), ("IS Mean", "inception_score_mean"), ("IS Std", "inception_score_std"), ("KID", "kid")]
    if not math.isnan(gen.get("precision", float("nan"))):
        names += [("Precision", "precision"), ("Recall", "recall")]
    _table("GENERATIVE METRICS", [(n, _fmt(gen.get(k, float("nan")), k)) for n, k in names])
    print("=" * 80 + "\n")


def evaluate_main(argv=None):
    a = evaluate_parser().parse_args(argv)
    if a.seed is not None:
        train.set_seed(a.seed)
    device = _device(a.device)
    net, run_args = checkpoint.load_run(a.model_path, device, dataset=a.dataset, arch=a.arch, data_dir=a.data_dir)
    L.set_compute_dtype(getattr(run_args, "dtype", "fp32"))
    _, test_ds, _ = _dataset(run_args, a.dataset, a.data_dir)
    ev = _with(run_args, batch_size=a.batch_size, num_workers=a.num_workers, max_fid_samples=a.max_fid_samples,
               max_gen_metrics_samples=a.max_gen_metrics_samples, prior_sampler=a.prior_sampler,
               pixelcnn_temperature=a.pixelcnn_temperature, gen_precision_recall=a.gen_precision_recall)
    ev.seed = a.seed
    loader = train.make_loader(test_ds, a.batch_size, device, ev, shuffle=False)
    print(f"Evaluating {run_args.arch} on {a.dataset}: {len(test_ds)} test images, {net.total_trainable_params():,} parameters")
    if a.max_fid_samples > 0:
        meters, recon = train.evaluate_with_recon_metrics(net, loader, device, ev)
    else:
        meters, recon = train.evaluate(net, loader, device, ev), dict(NAN_RESULT)
    losses = {k: m.avg for k, m in meters.items()}
    keys = list(net.objectives.keys())
    hv_fn = build_hv_indicator(keys, types.SimpleNamespace(hv_ref=None))  # evaluate.py:82-106: the fixed reference point 1.1
    hv = hv_fn([losses[k] for k in keys]) if hv_fn is not None else None
    gen = {k: float("nan") for k in train.GEN_METRIC_KEYS}
    if a.gen_metrics == "on":
        prior = checkpoint.load_prior(a.prior_path, net, run_args, device) if a.prior_path else None
        gen = train.evaluate_generative_metrics(net, loader, device, ev, prior=prior)
    print_results_table(losses, recon, gen, hv)
    return {"test_losses": losses, "hv": hv, "recon_metrics": recon, "generative_metrics": gen, "arch": run_args.arch,
            "dataset": a.dataset, "model_path": a.model_path}


# ---- train_prior.py -------------------------------------------------------------------------------------------------------------------
def train_prior_parser():
    p = ArgumentParser(description="Train a PixelCNN prior on the codes of a saved VQ autoencoder (flat or hierarchical)")
    p.add_argument("--checkpoint", "--vqvae_checkpoint", "--vqvae2_checkpoint", dest="checkpoint", type=str, required=True)
    p.add_argument("--dataset", type=str, default=None, help="default: the run's")
    p.add_argument("--data_dir", type=str, default=None)
    p.add_argument("--batch_size", type=int, default=None)
    p.add_argument("--epochs", type=int, default=None)
    p.add_argument("--lr", type=float, default=None)
    p.add_argument("--hidden_channels", type=int, default=None)
    p.add_argument("--num_layers", type=int, default=None)
    p.add_argument("--temperature", type=float, default=None)
    p.add_argument("--num_samples", type=int, default=None, help="images of the final 'with prior' grid")
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--device", type=str, default=_DEVICE)
    p.add_argument("--prior_loader", type=str, default=None, choices=list(_prior.PRIOR_LOADERS))
    p.add_argument("--prior_step", type=str, default=None, choices=list(_prior.PRIOR_STEPS))
    p.add_argument("--prior_sampler", type=str, default=None, choices=_SAMPLERS)
    p.add_argument("--output_dir", type=str, default=None, help="default: the checkpoint's run directory")
    return p


def train_prior_main(argv=None):
    a = train_prior_parser().parse_args(argv)
    if a.seed is not None:
        train.set_seed(a.seed)
    device = _device(a.device)
    net, run_args = checkpoint.load_run(a.checkpoint, device, dataset=a.dataset, data_dir=a.data_dir)
    if not train._is_vq_arch(run_args.arch):
        raise ValueError(f"a prior is trained over VQ codes; the checkpoint's architecture is {run_args.arch!r}")
    L.set_compute_dtype(getattr(run_args, "dtype", "fp32"))
    ns = _with(run_args, batch_size=a.batch_size, pixelcnn_epochs=a.epochs, pixelcnn_lr=a.lr, pixelcnn_hidden_channels=a.hidden_channels,
               pixelcnn_num_layers=a.num_layers, pixelcnn_temperature=a.temperature, num_vis_samples=a.num_samples, seed=a.seed,
               prior_loader=a.prior_loader, prior_step=a.prior_step, prior_sampler=a.prior_sampler)
    ns.prior_type = "pixelcnn"
    train_ds, _, _ = _dataset(run_args, a.dataset, a.data_dir)
    loader = train.make_loader(train_ds, ns.batch_size, device, ns, shuffle=True)
    out_dir = a.output_dir or checkpoint.run_dir_of(a.checkpoint)
    _prior.train_pixelcnn_prior(net, loader, device, ns, out_dir)
    prior_dir = os.path.join(out_dir, "pixelcnn_prior")
    # what load_prior needs to rebuild this prior, should it differ from the run's own flags (the reference keeps them under 'args' too)
    hyper = {"hidden_channels": ns.pixelcnn_hidden_channels, "num_layers": ns.pixelcnn_num_layers}
    for name in checkpoint.PRIOR_FILES:
        f = os.path.join(prior_dir, "checkpoints", name)
        ck = torch.load(f, map_location="cpu", weights_only=True)
        ck["args"] = hyper
        torch.save(ck, f)
    grid_path = os.path.join(out_dir, "figures", "generated", "final_random_samples_with_prior.png")
    visual.write_random_samples(_prior.LAST_RUN["samples_device"], grid_path)
    return {"prior_dir": prior_dir, "epoch_losses": list(_prior.LAST_RUN["epoch_losses"]), "grid": grid_path}


# ---- generate_samples.py --------------------------------------------------------------------------------------------------------------
def generate_samples_parser():
    p = ArgumentParser(description="Draw images from a saved run: through a trained prior, or from the model's own sample()")
    p.add_argument("--checkpoint", "--vqvae_checkpoint", "--vqvae2_checkpoint", dest="checkpoint", type=str, required=True)
    p.add_argument("--prior_checkpoint", type=str, default=None, help="a prior checkpoint or the run directory that holds one")
    p.add_argument("--num_samples", type=int, default=64)
    p.add_argument("--temperature", type=float, default=1.0)
    p.add_argument("--batch_size", type=int, default=64)
    p.add_argument("--output_dir", type=str, default="generated_samples")
    p.add_argument("--device", type=str, default=_DEVICE)
    p.add_argument("--save_grid", action="store_true")
    p.add_argument("--grid_nrow", type=int, default=8)
    p.add_argument("--prior_sampler", type=str, default="full", choices=_SAMPLERS)
    p.add_argument("--seed", type=int, default=None)
    return p


def decoder_value_range(net):
    """(-1, 1) behind a tanh decoder, else (0, 1) (generate_samples_pixelcnn_vqvae.py:172-173)."""
    act = getattr(net, "recons_activation", None)
    names = [type(act).__name__] if isinstance(act, torch.nn.Module) else [type(m).__name__ for m in net.modules()]
    return (-1.0, 1.0) if "Tanh" in names else (0.0, 1.0)


@torch.no_grad()
def generate_samples_main(argv=None):
    a = generate_samples_parser().parse_args(argv)
    if a.num_samples <= 0 or a.batch_size <= 0:
        raise ValueError("--num_samples and --batch_size must be positive")
    device = _device(a.device)
    net, run_args = checkpoint.load_run(a.checkpoint, device)
    L.set_compute_dtype(getattr(run_args, "dtype", "fp32"))
    prior = checkpoint.load_prior(a.prior_checkpoint, net, run_args, device) if a.prior_checkpoint else None
    if a.seed is not None:
        train.set_seed(a.seed)
    value_range = decoder_value_range(net)
    os.makedirs(a.output_dir, exist_ok=True)
    tag = f"temp{a.temperature:.2f}"
    batches, files = [], []
    single_dir = os.path.join(a.output_dir, f"individual_{tag}")
    for start in range(0, a.num_samples, a.batch_size):
        b = min(a.batch_size, a.num_samples - start)
        if prior is not None:
            x = _prior.generate_samples_vq_with_prior(net, prior, b, device, temperature=a.temperature,
                                                      cached=_prior.PRIOR_SAMPLERS[a.prior_sampler])
        else:
            x = net.sample(num_samples=b, device=device)
        if a.save_grid:
            batches.append(x.float())
            continue
        u8 = visual.to_uint8_batch(x, normalize=True, value_range=value_range).cpu()  # the batch's one copy to the host
        for i in range(b):
            files.append(os.path.join(single_dir, f"sample_{start + i:05d}.png"))
            visual.save_u8(u8[i], files[-1])
    if a.save_grid:
        files.append(os.path.join(a.output_dir, f"samples_grid_{tag}.png"))
        visual.save_grid(torch.cat(batches), files[-1], nrow=a.grid_nrow, normalize=True, value_range=value_range)
    print(f"wrote {len(files)} file(s) under {a.output_dir}")
    return {"files": files, "value_range": value_range, "num_samples": a.num_samples}

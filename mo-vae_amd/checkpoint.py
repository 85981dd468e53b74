"""Reading a run back (reference evaluate.py:20-79 and the loaders of its sampling tools): the autoencoder from
`checkpoints/final_checkpoint.pth`, the prior from `pixelcnn_prior/` or `pixelsnail_prior/` next to it.

train.main writes the checkpoint with the reference's keys plus `input_size`, so a run is rebuilt from the file alone; a checkpoint
without that key (the reference's) takes the image side from the dataset, as the reference does.
"""
import os
import re
import types
import warnings

import torch

from . import prior as _prior
from .models import get_network

AUTOENCODER_FILE = os.path.join("checkpoints", "final_checkpoint.pth")
PRIOR_DIRS = {"pixelcnn_prior": False, "pixelsnail_prior": True}  # directory -> is PixelSNAIL
PRIOR_FILES = ("best_prior.pth", "final_prior.pth")               # a run directory's prior: the best one, else the last


def _read(path, device):
    if not os.path.exists(path):
        raise FileNotFoundError(f"checkpoint not found: {path}")
    return torch.load(path, map_location=device, weights_only=True)


def run_dir_of(checkpoint_path):
    """<run>/checkpoints/final_checkpoint.pth -> <run> (a file elsewhere: its own directory)."""
    d = os.path.dirname(os.path.abspath(checkpoint_path))
    return os.path.dirname(d) if os.path.basename(d) == "checkpoints" else d


def load_run(path, device, dataset=None, arch=None, data_dir=None):
    """evaluate.py:20-79 -> (net in eval mode on `device`, args namespace of the run).  `path`: the checkpoint file or the run
    directory that holds checkpoints/final_checkpoint.pth.  `dataset` / `data_dir` override the run's (they matter only for a
    checkpoint without `input_size`); an `arch` that differs from the checkpoint's is warned about and the checkpoint's is used.
    A checkpoint this build wrote is loaded strictly; a state_dict whose checkpoint lacks the keys this build writes (the
    reference's) is loaded with strict=False and the keys that did not match are printed.  ValueError without `args`."""
    if os.path.isdir(path):
        path = os.path.join(path, AUTOENCODER_FILE)
    ckpt = _read(path, device)
    if not isinstance(ckpt, dict) or not isinstance(ckpt.get("args"), dict):
        raise ValueError(f"{path} does not contain 'args': the model's configuration cannot be rebuilt")
    args = types.SimpleNamespace(**ckpt["args"])
    if arch is not None and hasattr(args, "arch") and str(args.arch).lower() != str(arch).lower():
        warnings.warn(f"checkpoint arch ({args.arch}) does not match the given arch ({arch}); using the checkpoint's")
    if not hasattr(args, "arch"):
        if arch is None:
            raise ValueError(f"{path}: neither the checkpoint's args nor the call names an architecture")
        args.arch = arch
    own = "train_history" in ckpt  # the key only this build writes (also before it saved input_size)
    if "input_size" in ckpt:
        input_size = int(ckpt["input_size"])
    else:
        from .train import get_dataset

        name = dataset if dataset is not None else getattr(args, "dataset", None)
        if name is None:
            raise ValueError(f"{path} has no 'input_size' and no dataset is named to take the image side from")
        _, _, input_size = get_dataset(name, data_dir=data_dir if data_dir is not None else getattr(args, "data_dir", "./data"),
                                       normalize=getattr(args, "normalize_inputs", getattr(args, "normalize", False)),
                                       max_items=getattr(args, "max_items", None))
    device = torch.device(device)
    net = get_network(input_size, num_channels=3, args=args, device=device).to(device)
    state = ckpt.get("model_state_dict", None)
    if state is None:
        raise ValueError(f"{path} does not contain 'model_state_dict'")
    res = net.load_state_dict(state, strict=own)
    if res.missing_keys or res.unexpected_keys:
        print(f"load_run: missing keys {list(res.missing_keys)}, unexpected keys {list(res.unexpected_keys)}")
    net.eval()
    args.input_size = input_size
    return net, args


def _is_snail_state(state):
    return any(re.search(r"(^|\.)blocks\.\d+\.", k) for k in state)


def find_prior(run_dir_or_file):
    """-> (file, is PixelSNAIL or None when the path does not say).  A run directory is searched for pixelcnn_prior/ then
    pixelsnail_prior/, best_prior.pth before final_prior.pth."""
    p = os.path.abspath(run_dir_or_file)
    if os.path.isdir(p):
        roots = [p] if os.path.basename(p) in PRIOR_DIRS else [os.path.join(p, d) for d in PRIOR_DIRS]
        for root in roots:
            for name in PRIOR_FILES:
                f = os.path.join(root, "checkpoints", name)
                if os.path.exists(f):
                    return f, PRIOR_DIRS[os.path.basename(root)]
        raise FileNotFoundError(f"no prior checkpoint under {p} ({' or '.join(PRIOR_DIRS)}/checkpoints/{' or '.join(PRIOR_FILES)})")
    for part in p.split(os.sep)[::-1]:
        if part in PRIOR_DIRS:
            return p, PRIOR_DIRS[part]
    return p, None


def load_prior(run_dir_or_file, net, args, device):
    """The prior of a run, in eval mode: PixelCNN / HierarchicalPixelCNN or their PixelSNAIL forms, chosen by the checkpoint's directory
    (pixelcnn_prior/ or pixelsnail_prior/; a bare file: by its state_dict's keys), built with the run's hyper-parameters (`args`) for
    `net`'s codebook and loaded strictly."""
    path, snail = find_prior(run_dir_or_file)
    ckpt = _read(path, device)
    state = ckpt["model_state_dict"] if isinstance(ckpt, dict) and "model_state_dict" in ckpt else ckpt
    if snail is None:
        snail = _is_snail_state(state)
    hyper = ckpt.get("args") if isinstance(ckpt, dict) else None
    if isinstance(hyper, dict):  # a prior trained apart from the run (train_prior.py) names what it was built with
        args = types.SimpleNamespace(**{**vars(args),
                                        "pixelcnn_hidden_channels": hyper.get("hidden_channels", getattr(args, "pixelcnn_hidden_channels", 128)),
                                        "pixelcnn_num_layers": hyper.get("num_layers", getattr(args, "pixelcnn_num_layers", 15))})
    if snail:
        prior = _prior.build_pixelsnail_prior(net, args, device)
    else:  # (not through build_prior's --prior_type switch, which refuses pixelsnail by name)
        prior = _prior.build_prior(net, types.SimpleNamespace(**{**vars(args), "prior_type": "pixelcnn"}), device)
    prior.load_state_dict(state, strict=True)
    prior.eval()
    return prior

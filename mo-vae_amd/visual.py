"""Pictures of a run (reference main.py:511-656): image grids made on the device, written as PNG.

`image_grid` is torchvision's make_grid followed by save_image's quantisation as ONE C-ABI call (include/movae.h:
movae_image_grid_u8; csrc/visual.hip): a float image batch, read through its strides, becomes the finished uint8 picture [H, W, 3] on
the device, so the only thing the host ever copies is the picture's bytes.  `to_uint8_batch` is the same call with one image per
grid row and no padding: the per-image dump.  `generate_random_samples` / `generate_reconstructed_samples` keep the reference's
signatures and return values; the file they write is the grid itself (the reference's matplotlib figure around it -- title, row
labels, 150 dpi -- is not reproduced).
"""
import math
import os

import torch

from . import _lib as L

GRID_RAW, GRID_RANGE, GRID_MINMAX = 0, 1, 2  # include/movae.h: MOVAE_GRID_*


def grid_shape(n, h, w, nrow=8, padding=2):
    """(H, W) of the picture of n images of h x w: make_grid's geometry (a single image is returned as it is)."""
    if n <= 0 or h <= 0 or w <= 0 or nrow <= 0 or padding < 0:
        raise ValueError(f"grid_shape: n {n}, h {h}, w {w}, nrow {nrow} must be positive and padding {padding} non-negative")
    if n == 1:
        return h, w
    xmaps = min(nrow, n)
    ymaps = -(-n // xmaps)
    return ymaps * (h + padding) + padding, xmaps * (w + padding) + padding


def _images(x):
    L.require_gpu(x)
    if x.dim() == 3:
        x = x.unsqueeze(0)
    if x.dim() != 4 or x.size(1) not in (1, 3) or x.numel() == 0:
        raise ValueError(f"expected non-empty (B, C, H, W) images with C in (1, 3), got shape {tuple(x.shape)}")
    return x.detach() if x.dtype == torch.float32 else x.detach().float()


def image_grid(x, nrow=8, padding=2, normalize=False, value_range=None, pad_value=0.0):
    """make_grid(x, nrow, padding, normalize, value_range, pad_value) as save_image would write it: a uint8 [H, W, 3] device tensor.
    normalize=True without a value_range uses the minimum and maximum of the whole batch, found on the device.  One call into the
    library, no host sync; x is read through its strides (NCHW, channels_last, sliced views: no copy)."""
    x = _images(x)
    n, c, h, w = x.shape
    lo = hi = 0.0
    mode = GRID_RAW
    if normalize:
        mode = GRID_MINMAX
        if value_range is not None:
            lo, hi = float(value_range[0]), float(value_range[1])
            if not hi >= lo:
                raise ValueError(f"value_range {value_range!r}: the upper end is below the lower one")
            mode = GRID_RANGE
    H, W = grid_shape(n, h, w, nrow, padding)
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=x.device)
    ws_ptr, ws_bytes = 0, 0
    if mode == GRID_MINMAX:
        need = L.load().movae_image_grid_ws_bytes(n, c, h, w)
        ws = L.workspace(x.device)
        if ws.numel() < need:
            raise RuntimeError(f"image_grid: the workspace holds {ws.numel()} bytes, {need} are needed")
        ws_ptr, ws_bytes = ws.data_ptr(), ws.numel()
    L.call("movae_image_grid_u8", x.data_ptr(), *x.stride(), n, c, h, w, int(nrow), int(padding), float(pad_value), mode, lo, hi,
           out.data_ptr(), ws_ptr, ws_bytes, L.stream_ptr(x.device))
    return out


def to_uint8_batch(x, normalize=False, value_range=None):
    """Every image of the batch as bytes, uint8 [n, h, w, 3] on the device: the grid with one image per row and no padding, so the
    whole batch is one launch (pair) and one later copy.  The range of normalize=True without a value_range is the batch's."""
    x = _images(x)
    n, _, h, w = x.shape
    return image_grid(x, nrow=1, padding=0, normalize=normalize, value_range=value_range).reshape(n, h, w, 3)


def _pil():
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("writing a picture needs Pillow (the PIL module), which is not installed; image_grid / to_uint8_batch "
                           "give the bytes without it") from e
    return Image


def save_u8(u8, path):
    """One uint8 [H, W, 3] picture (device or host) -> `path`, in the format of its suffix: one copy to the host, then PIL."""
    Image = _pil()
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    Image.fromarray(u8.cpu().numpy()).save(path)


def save_grid(x, path, **kw):
    """image_grid(x, **kw) written to `path`; returns the grid (on the device)."""
    grid = image_grid(x, **kw)
    save_u8(grid, path)
    return grid


def _log_wandb(key, grid, epoch, step):
    try:
        import wandb
    except ImportError:
        return
    wandb.log({key: wandb.Image(grid.cpu().numpy(), caption=f"Epoch {epoch}")}, step=step)


@torch.no_grad()
def generate_random_samples(net, num_samples, device, save_path=None, log_to_wandb=False, epoch=None, step=None, prior=None,
                            temperature=1.0, prior_sampler="full"):
    """main.py:511-554 -> the samples (num_samples, C, H, W), on the device.  With `prior` the codes are drawn from it (through
    --prior_sampler's path), else net.sample.  The grid has int(sqrt(num_samples)) images per row, normalised to the batch's range."""
    if prior is not None:
        from . import prior as _prior

        samples = _prior.generate_samples_vq_with_prior(net, prior, num_samples, device, temperature=temperature,
                                                        cached=_prior.PRIOR_SAMPLERS[prior_sampler])
    else:
        samples = net.sample(num_samples=num_samples, device=device)
    write_random_samples(samples, save_path, log_to_wandb, epoch, step)
    return samples


def write_random_samples(samples, save_path=None, log_to_wandb=False, epoch=None, step=None):
    """The picture of generate_random_samples for samples already drawn."""
    if save_path is None and not (log_to_wandb and epoch is not None):
        return None
    grid = image_grid(samples, nrow=max(1, int(math.sqrt(samples.size(0)))), normalize=True)
    if save_path is not None:
        save_u8(grid, save_path)
    if log_to_wandb and epoch is not None:
        _log_wandb("generated_samples", grid, epoch, step)
    return grid


def first_items(loader, num_samples, device):
    """The first `num_samples` images of the loader's SET, on the device, without iterating the loader: a ResidentLoader assembles
    rows 0 .. n-1 of its resident set, anything else with a `.dataset` is indexed item by item; neither advances an epoch's order
    nor draws from a generator.  Only a loader without a set is iterated."""
    from .data import ResidentLoader

    ds = getattr(loader, "dataset", None)
    if ds is not None:
        n = min(int(num_samples), len(ds))
        if isinstance(loader, ResidentLoader):
            loader._device_indices()  # (makes the set resident on first use; the epoch's list is cached, not consumed)
            batch = loader._batch(torch.arange(n, dtype=torch.int32, device=loader.device))
            return (batch[0] if isinstance(batch, (tuple, list)) else batch).to(device)
        return torch.stack([ds[i][0] for i in range(n)]).to(device)
    got, have = [], 0
    for images, _ in loader:
        got.append(images[: num_samples - have].to(device))
        have += got[-1].size(0)
        if have >= num_samples:
            break
    return torch.cat(got)


@torch.no_grad()
def generate_reconstructed_samples(net, split_name, loader, num_samples, device, save_path=None, log_to_wandb=False, epoch=None,
                                   step=None):
    """main.py:557-656 -> (originals, reconstructions), both (num_samples, C, H, W) on the device.  The picture has the originals in
    its upper row and the reconstructions below (nrow = num_samples, one value range over both, white padding); the two halves are
    concatenated on the device.  KeyError when the model's outputs have no 'recons'."""
    net.eval()
    originals = first_items(loader, num_samples, device)
    recon = net(originals).get("recons")
    if recon is None:
        raise KeyError("Model output dictionary must contain 'recons'.")
    recon = recon.detach()
    if save_path is not None or (log_to_wandb and epoch is not None):
        grid = image_grid(torch.cat([originals.float(), recon.float()], dim=0), nrow=num_samples, normalize=True, pad_value=1.0)
        if save_path is not None:
            save_u8(grid, save_path)
        if log_to_wandb and epoch is not None:
            _log_wandb(f"reconstructed_{split_name}_samples", grid, epoch, step)
    return originals, recon


def epoch_figure_paths(save_root, epoch):
    """The three files of one --vis pass."""
    stem = f"epoch_{epoch:04d}"
    return {"random": os.path.join(save_root, "figures", "generated", f"{stem}_random_samples.png"),
            "test": os.path.join(save_root, "figures", "reconstructed", f"{stem}_test_samples.png"),
            "train": os.path.join(save_root, "figures", "reconstructed", f"{stem}_train_samples.png")}


def write_epoch_figures(net, train_loader, test_loader, device, args, save_root, epoch, step=None, log_to_wandb=False):
    """One --vis pass (main.py:1391-1420): random samples and the test / train reconstructions of `epoch`.  It leaves the training
    trajectory alone: the generators of the host and of the device are forked around it, net.training is restored, and the loaders
    are read through first_items (no iteration, no epoch advanced).  Nothing of a captured step is touched: the pass launches eager
    inference calls only."""
    n = int(getattr(args, "num_vis_samples", 4))
    paths = epoch_figure_paths(save_root, epoch)
    was_training = net.training
    dev = torch.device(device)
    # the device-side counters a forward may advance (capture._state_tensors: BetaTC's step counter, the in-kernel noise generator's
    # {seed, draws}): put back afterwards, in stream order, at the addresses a captured step points at
    counters = [(t, t.clone()) for t in (getattr(net, "_iter_dev", None), getattr(net, "_noise_state_t", None)) if isinstance(t, torch.Tensor)]
    try:
        with torch.random.fork_rng(devices=[dev]):
            net.eval()
            generate_random_samples(net, n, dev, save_path=paths["random"], log_to_wandb=log_to_wandb, epoch=epoch, step=step)
            generate_reconstructed_samples(net, "test", test_loader, n, dev, save_path=paths["test"], log_to_wandb=log_to_wandb,
                                           epoch=epoch, step=step)
            generate_reconstructed_samples(net, "train", train_loader, n, dev, save_path=paths["train"], log_to_wandb=log_to_wandb,
                                           epoch=epoch, step=step)
    finally:
        with torch.no_grad():
            for t, saved in counters:
                t.copy_(saved)
        net.train(was_training)
    return paths

"""Prior stage that follows VQ-VAE training -- drop-in for the reference's main.py:890-1085 (train_pixelcnn_prior,
generate_samples_vq_with_prior) on the HIP kernels.

The reference extracts every training image's code grid once into an LMDB file (utils/vq_codes_lmdb.py:20-103) and trains the
prior from a Dataset over it (:106-172).  `lmdb` is not importable here (and its on-disk format is a pickle per sample), so the
cache is kept IN MEMORY: `VQCodeDataset` has the reference Dataset's `__len__` / `__getitem__` contract (a long tensor `z`, or a
pair `(z_top, z_bottom)` for the hierarchical models) -- parity unpinned as a storage format, the tensors it yields are the
golden-pinned models' own outputs.  `--no_prior_lmdb_codes` re-extracts the codes on the fly each batch, like the reference.

Opt-in: `--prior_loader device` keeps the cache on the device and assembles each batch in one launch
(DeviceCodeLoader), `--prior_step graph` replays the optimisation step as one hipGraph (GraphedPriorStep; PixelCNN priors only).
"""
import os

import torch

from . import capture
from . import ops
from .data import ResidentLoader, refuse_if_too_big
from .models.pixelcnn_prior import HierarchicalPixelCNN, HierarchicalPixelSNAIL, PixelCNN, PixelSNAIL
from .optim import FusedAdam, clip_grad_norm_

#: what the last train_pixelcnn_prior call did (tests and callers that want the numbers; the reference only prints them)
LAST_RUN = {}
#: data.refuse_if_too_big's wording for a code store
_TOO_BIG = ("the code grids need", "keep them on the host with --prior_loader host")


class VQCodeDataset(torch.utils.data.Dataset):
    """utils/vq_codes_lmdb.py:106-172 without the file: item i is the code grid(s) of training sample i."""

    def __init__(self, codes, is_hierarchical, transform_index=None):
        self.is_hierarchical, self.transform_index = is_hierarchical, transform_index
        if is_hierarchical:
            self.z_top, self.z_bottom = codes
            assert self.z_top.size(0) == self.z_bottom.size(0)
            self.meta = {"is_hierarchical": True, "z_top_shape": tuple(self.z_top.shape[1:]),
                         "z_bottom_shape": tuple(self.z_bottom.shape[1:]), "dtype": "int64"}
        else:
            (self.z,) = codes
            self.meta = {"is_hierarchical": False, "z_shape": tuple(self.z.shape[1:]), "dtype": "int64"}

    def __len__(self):
        return (self.z_top if self.is_hierarchical else self.z).size(0)

    def __getitem__(self, idx):
        if idx < 0 or idx >= len(self):
            raise IndexError(f"Index {idx} not found in the code cache")
        t = self.transform_index
        if self.is_hierarchical:
            a, b = self.z_top[idx].long(), self.z_bottom[idx].long()
            return (t(a), t(b)) if t is not None else (a, b)
        z = self.z[idx].long()
        return t(z) if t is not None else z


@torch.no_grad()
def extract_codes(net, train_loader, device, is_hierarchical, on_device=False):
    """One pass of the frozen VQ model over the training set (utils/vq_codes_lmdb.py:47-93): code grids on the host, or with
    `on_device` left where the model wrote them (no .cpu() round trip; what DeviceCodeLoader gathers its batches from)."""
    net.eval()
    tops, bots = [], []
    # held as int16 / int32 (a code is < num_embeddings): an int64 grid per ImageNet-scale VQ-VAE-2 sample would be
    # ~50 GB where the reference spills to LMDB; VQCodeDataset.__getitem__ hands out .long() like the reference's Dataset
    store = torch.int16 if int(getattr(net, "num_embeddings", 1 << 20)) <= (1 << 15) else torch.int32
    keep = (lambda t: t.to(store)) if on_device else (lambda t: t.to(store).cpu())
    sized = False
    for images, _ in train_loader:
        images = images.to(device)
        if is_hierarchical:
            cd = net.get_code_indices(images)
            tops.append(keep(cd["indices_top"]))
            bots.append(keep(cd["indices_bottom"]))
        else:
            tops.append(keep(net.get_code_indices(images)))
        if on_device and not sized:  # refuse before the set is resident, not after: the first batch gives the bytes per sample
            sized = True
            per = sum(t[-1][0].numel() * t[-1].element_size() for t in (tops, bots) if t)
            try:
                total = len(train_loader.dataset)
            except (AttributeError, TypeError):
                total = tops[0].size(0)
            refuse_if_too_big(2 * per * total, tops[0].device, *_TOO_BIG)  # twice: the pieces and, for a moment, their concatenation
    if is_hierarchical:
        return VQCodeDataset((torch.cat(tops), torch.cat(bots)), True)
    return VQCodeDataset((torch.cat(tops),), False)


class DeviceCodeLoader(ResidentLoader):
    """data.ResidentLoader over the batches of a VQCodeDataset whose int16 / int32 grids are resident on the device (uploaded on first
    use when the dataset holds them on the host).  Every batch is ONE movae_codes_batch launch that gathers the rows of both levels
    and widens them to int64.  Yields z for a flat dataset, (z_top, z_bottom) for a hierarchical one.

    bind(out_top, out_bottom): full batches are written into these buffers (a captured step's static inputs) and the buffers
    themselves are yielded -- valid until the next batch; without it every batch is a fresh tensor."""

    noun = "code grids"

    def __init__(self, ds, batch_size, device, shuffle=True, seed=0):
        if not isinstance(ds, VQCodeDataset):
            raise TypeError(f"DeviceCodeLoader needs a VQCodeDataset, got {type(ds).__name__}")
        if ds.transform_index is not None:
            raise TypeError("DeviceCodeLoader: a dataset with a per-item transform_index needs the host loader")
        super().__init__(ds, batch_size, device, shuffle, seed=seed)
        self._stores = None
        self._out = (None, None)

    def bind(self, out_top, out_bottom=None):
        self._out = (out_top, out_bottom)

    def _upload(self):
        ds = self.dataset
        grids = [ds.z_top, ds.z_bottom] if ds.is_hierarchical else [ds.z]
        for g in grids:
            if g.dim() != 3 or g.dtype not in (torch.int16, torch.int32, torch.int64):
                raise ValueError(f"DeviceCodeLoader: code grids are integer [N][H][W], got {g.dtype} {tuple(g.shape)}")
        dt = torch.int16 if all(g.dtype == torch.int16 for g in grids) else torch.int32
        need = sum(g.numel() * (2 if dt == torch.int16 else 4) for g in grids if not g.is_cuda or g.dtype != dt)
        if need:
            refuse_if_too_big(need, self.device, *_TOO_BIG)
        self._stores = [g.to(device=self.device, dtype=dt).contiguous() for g in grids]

    def _checked(self, idx):
        return ops.check_rows(idx, len(self.dataset))  # ValueError

    def _batch(self, rows):
        top, bottom = self._stores[0], (self._stores[1] if len(self._stores) == 2 else None)
        out_top, out_bottom = self._out if rows.numel() == self.batch_size else (None, None)
        return ops.codes_batch(top, rows, bottom, out_top=out_top, out_bottom=out_bottom)


def _one_step(prior, opt, z_top, z_bottom=None):
    """One optimisation step of the prior (main.py:996-1016) -> the step's loss, a device scalar."""
    opt.zero_grad()
    if z_bottom is not None:
        loss = prior.loss_function(z_top, z_bottom)["total_loss"]
    else:
        loss = prior.loss(z_top)  # == F.cross_entropy(logits.permute(0,2,3,1).reshape(-1,K), z.reshape(-1)), main.py:1003
    loss.backward()
    clip_grad_norm_(prior.parameters(), max_norm=1.0)
    opt.step()
    return loss.detach()


class GraphedPriorStep:
    """_one_step captured ONCE into a hipGraph and replayed per full batch, by the protocol of capture.py that train.GraphedTrainStep
    follows too: zero_grad, the loss, its backward, clip_grad_norm_(max_norm=1.0) and the FusedAdam(device_step=True) step are a few
    hundred short launches and a replay is one submission.  PixelCNN and HierarchicalPixelCNN only: they draw nothing in training, so
    the graph holds exactly the launches the eager step makes.  The warm-up steps a capture needs are rewound (capture.snapshot /
    restore): the first replay is step 1 of the stage, as the eager loop makes it.

    step(z_top, z_bottom=None) -> the step's loss (a fresh device scalar).  A batch of the captured shape replays -- with one copy_
    per level, or none when the batch IS the static input (DeviceCodeLoader.bind(step.static_top, step.static_bottom)); a batch of
    any other shape (the ragged last one) takes the eager step on the same optimizer state."""

    def __init__(self, prior, opt, example_top, example_bottom=None, warmup=3, record_calls=False):
        if isinstance(prior, (PixelSNAIL, HierarchicalPixelSNAIL)) or not isinstance(prior, (PixelCNN, HierarchicalPixelCNN)):
            raise NotImplementedError(f"{type(prior).__name__}: only PixelCNN / HierarchicalPixelCNN replay (PixelSNAIL counts its dropout "
                                      "draws in a host integer, which a capture would freeze); use the eager step")
        if not isinstance(opt, FusedAdam) or not opt._device_step:
            raise ValueError("GraphedPriorStep needs FusedAdam(device_step=True): the step counter must live on the device")
        if isinstance(prior, HierarchicalPixelCNN) != (example_bottom is not None):
            raise ValueError("GraphedPriorStep: a hierarchical prior takes (z_top, z_bottom), a flat one z alone")
        if warmup < 1:
            raise ValueError("GraphedPriorStep: at least one warm-up step (it creates the optimizer state the graph points at)")
        self.prior, self.opt = prior, opt
        self.replayed_steps = self.eager_steps = 0
        dev = example_top.device
        prior.train()
        self.static_top = example_top.clone()
        self.static_bottom = example_bottom.clone() if example_bottom is not None else None
        step = lambda: _one_step(prior, opt, self.static_top, self.static_bottom)  # noqa: E731
        snap = capture.snapshot(prior, opt, dev)
        try:
            capture.warm_up(step, warmup, dev)
            self.graph = torch.cuda.CUDAGraph()
            opt.zero_grad(set_to_none=True)
            #: (name, args) of every C-ABI launch in the captured step (tools/prior_train_bench.py counts them)
            self.calls = []
            with capture.recording(self.calls if record_calls else None), capture.capturing(self.graph):
                self.loss = step()
        finally:
            capture.restore(snap, prior, opt, dev)

    def step(self, z_top, z_bottom=None):
        if z_top.shape != self.static_top.shape or (z_bottom is None) != (self.static_bottom is None) or \
                (z_bottom is not None and z_bottom.shape != self.static_bottom.shape):
            self.eager_steps += 1
            return _one_step(self.prior, self.opt, z_top, z_bottom)
        if z_top.data_ptr() != self.static_top.data_ptr():
            self.static_top.copy_(z_top, non_blocking=True)
        if z_bottom is not None and z_bottom.data_ptr() != self.static_bottom.data_ptr():
            self.static_bottom.copy_(z_bottom, non_blocking=True)
        self.opt.sync_hyper()  # lr schedulers change the host value between replays
        self.graph.replay()
        self.replayed_steps += 1
        return self.loss.clone()  # the graph's own scalar is overwritten by the next replay


def is_hierarchical_arch(arch):
    return (arch or "").lower() in ("vq_vae2", "gg_vq_vae2")


def build_prior(net, args, device):
    """main.py:917-957."""
    if getattr(args, "prior_type", "pixelcnn").lower() == "pixelsnail":
        raise NotImplementedError("--prior_type pixelsnail (causal self-attention, models/pixelcnn_prior.py:95-259) is outside the "
                                  "MI355X hot-path scope (SURVEY 8f.4 names the PixelCNN prior); use --prior_type pixelcnn")
    kw = dict(num_embeddings=net.num_embeddings, embedding_dim=net.embedding_dim,
              hidden_channels=getattr(args, "pixelcnn_hidden_channels", 128), num_layers=getattr(args, "pixelcnn_num_layers", 15))
    cls = HierarchicalPixelCNN if is_hierarchical_arch(getattr(args, "arch", "vae")) else PixelCNN
    return cls(**kw).to(device)


def build_pixelsnail_prior(net, args, device):
    """main.py:917-944 (the `use_pixelsnail` branches): PixelSNAIL, or HierarchicalPixelSNAIL for the two-level VQ models."""
    hidden = getattr(args, "pixelcnn_hidden_channels", 128)
    common = dict(num_embeddings=net.num_embeddings, embedding_dim=net.embedding_dim, hidden_channels=hidden,
                  num_res_blocks_per_layer=getattr(args, "pixelsnail_num_res_blocks", 2), num_heads=getattr(args, "pixelsnail_num_heads", 8),
                  dropout=getattr(args, "pixelsnail_dropout", 0.1))
    if is_hierarchical_arch(getattr(args, "arch", "vae")):
        return HierarchicalPixelSNAIL(num_blocks_top=getattr(args, "pixelsnail_num_blocks", 8),
                                      num_layers_bottom=getattr(args, "pixelcnn_num_layers", 15), **common).to(device)
    return PixelSNAIL(num_blocks=getattr(args, "pixelsnail_num_blocks", 8), **common).to(device)


PRIOR_LOADERS, PRIOR_STEPS = ("host", "device"), ("eager", "graph")


def prior_modes(args):
    """(--prior_loader, --prior_step) of a namespace; one that has neither attribute selects today's path, ("host", "eager")."""
    loader_mode, step_mode = getattr(args, "prior_loader", "host"), getattr(args, "prior_step", "eager")
    if loader_mode not in PRIOR_LOADERS or step_mode not in PRIOR_STEPS:
        raise ValueError(f"prior_loader is one of {PRIOR_LOADERS} and prior_step one of {PRIOR_STEPS}, got {loader_mode!r}, {step_mode!r}")
    return loader_mode, step_mode


def train_pixelcnn_prior(net, train_loader, device, args, save_root, prior=None):
    """main.py:890-1043.  Returns the trained prior (eval mode).  `prior`: an already built prior to train instead of the one
    build_prior makes (e.g. build_pixelsnail_prior's; a PixelSNAIL prior writes under pixelsnail_prior/, main.py:913)."""
    hier = is_hierarchical_arch(getattr(args, "arch", "vae"))
    epochs = getattr(args, "pixelcnn_epochs", 100)
    lr = getattr(args, "pixelcnn_lr", 3e-4)
    net.eval()
    for p in net.parameters():
        p.requires_grad = False
    snail = isinstance(prior, (PixelSNAIL, HierarchicalPixelSNAIL))
    name = "PixelSNAIL" if snail else "PixelCNN"
    prior_dir = os.path.join(save_root, "pixelsnail_prior" if snail else "pixelcnn_prior")
    os.makedirs(os.path.join(prior_dir, "checkpoints"), exist_ok=True)
    if prior is None:
        prior = build_prior(net, args, device)
    use_cache = getattr(args, "prior_use_lmdb_codes", True)
    loader_mode, step_mode = prior_modes(args)
    if loader_mode == "device" and not use_cache:
        print("--prior_loader device needs the cached codes; with --no_prior_lmdb_codes the codes are extracted on the fly")
        loader_mode = "host"
    if step_mode == "graph" and snail:
        print(f"--prior_step graph: {name} counts its dropout draws in a host integer, which a capture would freeze; "
              "taking the eager step")
        step_mode = "eager"
    # (a captured step needs its step counter and learning rate on the device; the eager default keeps the host counter)
    opt = FusedAdam(prior.parameters(), lr=lr, weight_decay=0.0, device_step=step_mode == "graph")
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=epochs, eta_min=1e-6)
    codes_loader, n_codes = None, 0
    if use_cache:
        ds = extract_codes(net, train_loader, device, hier, on_device=loader_mode == "device")
        n_codes = len(ds)
        if loader_mode == "device":
            codes_loader = DeviceCodeLoader(ds, args.batch_size, device, shuffle=True, seed=getattr(args, "seed", None) or 0)
        else:
            codes_loader = torch.utils.data.DataLoader(ds, batch_size=args.batch_size, shuffle=True, num_workers=0, drop_last=False)
    print(f"Training {name} prior for {epochs} epochs..." + (" (codes extracted once, held in memory)" if use_cache
                                                             else " (extracting codes on-the-fly)"))
    K = net.num_embeddings
    best, epoch_losses = float("inf"), []
    graphed, eager_steps = None, 0

    def one_step(z_top, z_bottom=None):
        nonlocal graphed, eager_steps
        if not hier:
            z_bottom = None
        if step_mode == "graph":
            if graphed is None and z_top.size(0) == args.batch_size:  # captured on the first full batch, at its shape
                graphed = GraphedPriorStep(prior, opt, z_top, z_bottom)
                if isinstance(codes_loader, DeviceCodeLoader):  # later full batches are gathered straight into the static inputs
                    codes_loader.bind(graphed.static_top, graphed.static_bottom)
            if graphed is not None:
                return graphed.step(z_top, z_bottom)
        eager_steps += 1
        return _one_step(prior, opt, z_top, z_bottom)

    def batches(epoch):
        """The epoch's (z_top, z_bottom or None) batches on the device, from whichever source the stage has."""
        if isinstance(codes_loader, DeviceCodeLoader):
            codes_loader.set_epoch(epoch)
            for batch in codes_loader:
                yield batch if hier else (batch, None)
        elif codes_loader is not None:  # the host DataLoader over the cache
            for batch in codes_loader:
                if hier:
                    yield batch[0].to(device), batch[1].to(device)
                else:
                    yield (batch if isinstance(batch, torch.Tensor) else batch[0]).to(device), None
        else:  # extracted on the fly
            for images, _ in train_loader:
                images = images.to(device)
                with torch.no_grad():
                    codes = net.get_code_indices(images)
                yield (codes["indices_top"], codes["indices_bottom"]) if hier else (codes, None)

    for epoch in range(1, epochs + 1):
        prior.train()
        # device scalars: read once per epoch, not once per step (the reference calls .item() every step)
        losses = [one_step(z_top, z_bottom) for z_top, z_bottom in batches(epoch)]
        sched.step()
        if hasattr(opt, "sync_hyper"):
            opt.sync_hyper()
        avg = float(torch.stack(losses).mean().item()) if losses else 0.0
        epoch_losses.append(avg)
        if avg < best:
            best = avg
            torch.save({"epoch": epoch, "model_state_dict": {k: v.contiguous() for k, v in prior.state_dict().items()}, "loss": best},
                       os.path.join(prior_dir, "checkpoints", "best_prior.pth"))
    torch.save({"model_state_dict": {k: v.contiguous() for k, v in prior.state_dict().items()}, "epoch": epochs},
               os.path.join(prior_dir, "checkpoints", "final_prior.pth"))
    print(f"{name} prior training complete. Best loss: {best:.4f}. Saved to {prior_dir}")
    prior.eval()
    samples = generate_samples_vq_with_prior(net, prior, getattr(args, "num_vis_samples", 4), device,
                                             getattr(args, "pixelcnn_temperature", 1.0),
                                             cached=PRIOR_SAMPLERS[getattr(args, "prior_sampler", "full")])
    LAST_RUN.clear()
    LAST_RUN.update(net=net, prior=prior, epoch_losses=epoch_losses, use_cache=use_cache, n_codes=n_codes, samples=samples.detach().cpu(),
                    samples_device=samples.detach(),  # the same draw where it was made (train.main's "with prior" grid)
                    num_embeddings=K, loader=loader_mode, step_mode=step_mode,
                    replayed_steps=graphed.replayed_steps if graphed is not None else 0,
                    eager_steps=eager_steps + (graphed.eager_steps if graphed is not None else 0))
    return prior


#: --prior_sampler -> the `cached` argument of the priors' sample()
PRIOR_SAMPLERS = {"full": False, "cached": True, "cached_kv": "kv"}


@torch.no_grad()
def generate_samples_vq_with_prior(net, prior, num_samples, device, temperature=1.0, cached=False):
    """main.py:1046-1085.  cached: sample the PixelCNN levels with one launch per code (sampling.py) instead of a forward per code;
    cached="kv": every level that can be cached, the PixelSNAIL levels through their K/V cache included."""
    net.eval()
    prior.eval()
    if hasattr(prior, "sample_with_vqvae2"):
        return prior.sample_with_vqvae2(vqvae2_model=net, batch_size=num_samples, device=device, temperature=temperature, cached=cached)
    s = net.latent_spatial_dim
    z = prior.sample(batch_size=num_samples, height=s, width=s, device=device, temperature=temperature, cached=cached)
    q = net.vq_layer.embed_code(z).permute(0, 3, 1, 2)
    return net.decode(q)

"""Using a saved run: checkpoint.load_run / load_prior, the three tools (evaluate.py, train_prior.py, generate_samples.py) and the
--vis pictures of train.main.  Every run here is tiny (synthetic_cifar10 cut by --max_items, --hidden_dims 16 32) and shared by the
tests that read it."""
import glob
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

REFERENCE_EVALUATE_ARGV = ["--arch", "vq_vae", "--dataset", "CIFAR10", "--model_path", "logs/run/checkpoints/final_checkpoint.pth",
                           "--device", "cuda:0", "--batch_size", "64", "--num_workers", "2", "--max_fid_samples", "1000",
                           "--max_gen_metrics_samples", "500", "--seed", "7"]


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_evaluate_parser_accepts_the_reference_argv_and_the_additions():
    import evaluate

    a = evaluate.build_parser().parse_args(REFERENCE_EVALUATE_ARGV)
    assert (a.arch, a.dataset, a.batch_size, a.num_workers, a.max_fid_samples, a.max_gen_metrics_samples, a.seed) == \
        ("vq_vae", "CIFAR10", 64, 2, 1000, 500, 7)
    assert (a.gen_metrics, a.prior_path, a.prior_sampler, a.pixelcnn_temperature, a.gen_precision_recall, a.data_dir) == \
        ("on", None, "full", 1.0, False, None)
    b = evaluate.build_parser().parse_args(REFERENCE_EVALUATE_ARGV + ["--data_dir", "d", "--prior_path", "p", "--prior_sampler", "cached",
                                                                     "--pixelcnn_temperature", "0.8", "--gen_metrics", "off",
                                                                     "--gen_precision_recall"])
    assert (b.data_dir, b.prior_path, b.prior_sampler, b.pixelcnn_temperature, b.gen_metrics, b.gen_precision_recall) == \
        ("d", "p", "cached", 0.8, "off", True)
    with pytest.raises(SystemExit):
        evaluate.build_parser().parse_args(["--arch", "vae"])  # --dataset and --model_path are required, as in the reference


def test_the_other_two_parsers():
    import generate_samples
    import train_prior

    for flag in ("--checkpoint", "--vqvae_checkpoint", "--vqvae2_checkpoint"):
        a = train_prior.build_parser().parse_args([flag, "c.pth", "--dataset", "CIFAR10", "--data_dir", "d", "--batch_size", "64", "--epochs", "3",
                                                   "--lr", "1e-3", "--hidden_channels", "32", "--num_layers", "4", "--temperature", "0.9",
                                                   "--num_samples", "9", "--seed", "2", "--device", "cuda:0", "--prior_loader", "device",
                                                   "--prior_step", "graph", "--prior_sampler", "cached", "--output_dir", "o"])
        assert (a.checkpoint, a.epochs, a.hidden_channels, a.num_layers, a.prior_loader, a.prior_step, a.output_dir) == \
            ("c.pth", 3, 32, 4, "device", "graph", "o")
    g = generate_samples.build_parser().parse_args(["--checkpoint", "c.pth", "--prior_checkpoint", "p.pth", "--num_samples", "10", "--temperature",
                                                    "0.7", "--batch_size", "4", "--output_dir", "o", "--device", "cuda:0", "--save_grid",
                                                    "--grid_nrow", "5", "--prior_sampler", "cached_kv", "--seed", "3"])
    assert (g.checkpoint, g.prior_checkpoint, g.num_samples, g.temperature, g.save_grid, g.grid_nrow, g.prior_sampler, g.seed) == \
        ("c.pth", "p.pth", 10, 0.7, True, 5, "cached_kv", 3)
    assert generate_samples.build_parser().parse_args(["--checkpoint", "c"]).prior_checkpoint is None


def test_load_run_needs_the_args_of_the_run(tmp_path):
    import movae_amd  # noqa: F401
    from movae_amd import checkpoint

    f = tmp_path / "bare.pth"
    torch.save({"model_state_dict": {"w": torch.zeros(2)}, "epoch": 1}, f)
    with pytest.raises(ValueError, match="args"):
        checkpoint.load_run(str(f), "cpu", dataset="synthetic_cifar10", arch="vae")
    with pytest.raises(FileNotFoundError):
        checkpoint.load_run(str(tmp_path / "absent.pth"), "cpu")
    assert checkpoint.run_dir_of(str(tmp_path / "run" / "checkpoints" / "final_checkpoint.pth")) == str(tmp_path / "run")
    assert checkpoint.find_prior(str(tmp_path / "run" / "pixelsnail_prior" / "checkpoints" / "best_prior.pth"))[1] is True
    assert checkpoint.find_prior(str(tmp_path / "run" / "pixelcnn_prior" / "checkpoints" / "best_prior.pth"))[1] is False
    assert checkpoint.find_prior(str(tmp_path / "somewhere" / "prior.pth"))[1] is None


# ---- the runs -------------------------------------------------------------------------------------------------------------------------
COMMON = ["--dataset", "synthetic_cifar10", "--hidden_dims", "16", "32", "--batch_size", "32", "--max_items", "128", "--device", "cuda:0",
          "--seed", "1"]
VAE = COMMON + ["--arch", "vae", "--latent_dim", "16", "--aggregator", "upgrad", "--max_fid_samples", "0"]
VQ = COMMON + ["--arch", "vq_vae", "--embedding_dim", "8", "--num_embeddings", "16", "--epochs", "1", "--eval_freq", "0", "--max_fid_samples", "0",
               "--pixelcnn_epochs", "1", "--pixelcnn_hidden_channels", "16", "--pixelcnn_num_layers", "2", "--pixelcnn_lr", "3e-3"]


def _run(save_path, argv):
    """One train.cli run -> (history, run directory, the live net)."""
    from movae_amd import train

    history = train.cli(argv + ["--save_path", str(save_path)])
    return history, train.LAST_RUN["save_root"], train.LAST_RUN["net"]


def _png(path):
    from PIL import Image

    with Image.open(path) as im:
        return np.array(im.convert("RGB"))


def _test_loader(device, batch_size=32):
    from movae_amd import train

    _, test_ds, _ = train.get_dataset("synthetic_cifar10", max_items=128)
    args = train.parse_args(VAE)
    return train.make_loader(test_ds, batch_size, device, args, shuffle=False)


@pytest.fixture(scope="module")
def vae_run(gpu_device, tmp_path_factory):
    import movae_amd  # noqa: F401

    # --graph off: the live net then draws its reparameterisation noise from torch's generator, as a loaded net does
    history, root, net = _run(tmp_path_factory.mktemp("vae"), VAE + ["--epochs", "1", "--graph", "off"])
    return {"history": history, "root": root, "net": net, "ckpt": os.path.join(root, "checkpoints", "final_checkpoint.pth")}


@pytest.fixture(scope="module")
def vq_bare_run(gpu_device, tmp_path_factory):
    """A vq_vae run without a prior, with the final evaluation over its 12 test images."""
    import movae_amd  # noqa: F401
    from movae_amd import train

    _, root, net = _run(tmp_path_factory.mktemp("vq_bare"), VQ + ["--skip_pixelcnn", "--max_fid_samples", "12"])
    return {"root": root, "net": net, "final": {k: dict(v) for k, v in train.LAST_FINAL.items()},
            "ckpt": os.path.join(root, "checkpoints", "final_checkpoint.pth")}


@pytest.fixture(scope="module")
def vq_run(gpu_device, tmp_path_factory):
    import movae_amd  # noqa: F401
    from movae_amd import prior as P

    _, root, net = _run(tmp_path_factory.mktemp("vq"), VQ + ["--vis", "on"])
    return {"root": root, "net": net, "prior": P.LAST_RUN["prior"], "ckpt": os.path.join(root, "checkpoints", "final_checkpoint.pth")}


@pytest.mark.gpu
def test_load_run_gives_back_the_live_net(gpu_device, vae_run):
    from movae_amd import checkpoint, train

    live = vae_run["net"]
    assert torch.load(vae_run["ckpt"], weights_only=True)["input_size"] == 32
    for path in (vae_run["ckpt"], vae_run["root"]):  # the file, or the run directory
        net, args = checkpoint.load_run(path, gpu_device)
        assert not net.training and (args.arch, args.input_size, args.hidden_dims) == ("vae", 32, [16, 32])
        want, got = live.state_dict(), net.state_dict()
        assert list(want) == list(got)
        for k in want:
            assert torch.equal(want[k], got[k]), k
    with pytest.warns(UserWarning, match="does not match"):
        other, args = checkpoint.load_run(vae_run["ckpt"], gpu_device, arch="vq_vae")
    assert args.arch == "vae" and type(other) is type(live)
    loader = _test_loader(gpu_device)
    torch.manual_seed(11)  # (a VAE's evaluation draws noise: both passes get the same stream)
    a = {k: m.avg for k, m in train.evaluate(net, loader, gpu_device, args).items()}
    torch.manual_seed(11)
    b = {k: m.avg for k, m in train.evaluate(live, loader, gpu_device, args).items()}
    assert a == b and all(math.isfinite(v) for v in a.values())  # the same kernels on the same bits in the same order


@pytest.mark.gpu
def test_evaluate_tool_repeats_the_final_evaluation(gpu_device, vq_bare_run, capsys):
    """On a vq_vae run: its evaluation draws no noise, so the tool must give the run's own final numbers exactly."""
    import evaluate
    from movae_amd import metrics as M

    final = vq_bare_run["final"]
    res = evaluate.main(["--arch", "vq_vae", "--dataset", "synthetic_cifar10", "--model_path", vq_bare_run["ckpt"], "--batch_size", "32",
                         "--max_fid_samples", "12", "--max_gen_metrics_samples", "8", "--seed", "1"])
    assert res["test_losses"] == final["losses"] and "codebook_usage_percentage" in res["test_losses"]
    assert res["recon_metrics"]["psnr"] == final["recon"]["psnr"] and res["recon_metrics"]["ssim"] == final["recon"]["ssim"]
    assert math.isfinite(res["recon_metrics"]["psnr"]) and math.isfinite(res["recon_metrics"]["ssim"])
    assert res["hv"] is not None and res["hv"] >= 0.0
    out = capsys.readouterr().out
    assert "RECONSTRUCTION METRICS" in out and "GENERATIVE METRICS" in out and "Hypervolume (HV)" in out
    if M._inception_weights() is None:
        assert math.isnan(res["recon_metrics"]["rfid"]) and all(math.isnan(v) for v in res["generative_metrics"].values())
        assert "N/A" in out


@pytest.mark.gpu
def test_prior_round_trip_and_generate_samples(gpu_device, vq_run, tmp_path):
    import generate_samples
    from movae_amd import checkpoint
    from movae_amd.models.pixelcnn_prior import PixelCNN
    from movae_amd.visual import grid_shape

    net, args = checkpoint.load_run(vq_run["ckpt"], gpu_device)
    final = os.path.join(vq_run["root"], "pixelcnn_prior", "checkpoints", "final_prior.pth")
    prior = checkpoint.load_prior(final, net, args, gpu_device)
    assert type(prior) is PixelCNN and not prior.training
    saved, got = torch.load(final, map_location=gpu_device, weights_only=True)["model_state_dict"], prior.state_dict()
    assert list(saved) == list(got) and all(torch.equal(saved[k], got[k]) for k in saved)  # what was written, bit for bit

    def masked(state):
        # a masked convolution zeroes the masked entries of its weight in place before each use: the file holds what the last Adam
        # step wrote there, the live prior (which has sampled since) zeros -- the entries that are ever used must agree
        return {k: v * state[k[:-6] + "mask"] if k.endswith("weight") and k[:-6] + "mask" in state else v for k, v in state.items()}

    want, got = masked(vq_run["prior"].state_dict()), masked(got)
    assert list(want) == list(got)
    for k in want:
        assert torch.equal(want[k], got[k]), k
    assert type(checkpoint.load_prior(vq_run["root"], net, args, gpu_device)) is PixelCNN  # the run directory: its best prior
    # the "with prior" grid of the run itself (--vis on): the four samples the stage drew, two per row
    with_prior = _png(os.path.join(vq_run["root"], "figures", "generated", "final_random_samples_with_prior.png"))
    assert with_prior.shape == (*grid_shape(4, 32, 32, 2, 2), 3)

    pictures = []
    for name in ("a", "b"):
        res = generate_samples.main(["--checkpoint", vq_run["ckpt"], "--prior_checkpoint", vq_run["root"], "--num_samples", "6", "--batch_size",
                                     "4", "--grid_nrow", "3", "--save_grid", "--seed", "3", "--output_dir", str(tmp_path / name)])
        assert [os.path.basename(f) for f in res["files"]] == ["samples_grid_temp1.00.png"]
        pictures.append(open(res["files"][0], "rb").read())
    assert pictures[0] == pictures[1]
    assert _png(res["files"][0]).shape == (*grid_shape(6, 32, 32, 3, 2), 3)
    # one file per image; without a prior the draw is net.sample
    res = generate_samples.main(["--checkpoint", vq_run["ckpt"], "--num_samples", "3", "--batch_size", "2", "--seed", "3", "--output_dir",
                                 str(tmp_path / "single")])
    assert [os.path.basename(f) for f in res["files"]] == [f"sample_{i:05d}.png" for i in range(3)]
    assert all(_png(f).shape == (32, 32, 3) for f in res["files"])


@pytest.mark.gpu
def test_train_prior_tool_on_a_run_without_a_prior(gpu_device, vq_bare_run):
    import train_prior
    from movae_amd import checkpoint
    from movae_amd.visual import grid_shape

    root = vq_bare_run["root"]
    assert not os.path.exists(os.path.join(root, "pixelcnn_prior"))
    res = train_prior.main(["--checkpoint", os.path.join(root, "checkpoints", "final_checkpoint.pth"), "--epochs", "2", "--hidden_channels", "24",
                            "--num_layers", "3", "--lr", "3e-3", "--num_samples", "4", "--seed", "2"])
    files = sorted(os.path.basename(f) for f in glob.glob(os.path.join(root, "pixelcnn_prior", "checkpoints", "*.pth")))
    assert files == ["best_prior.pth", "final_prior.pth"] and res["prior_dir"] == os.path.join(root, "pixelcnn_prior")
    assert len(res["epoch_losses"]) == 2 and np.isfinite(res["epoch_losses"]).all()
    assert _png(res["grid"]).shape == (*grid_shape(4, 32, 32, 2, 2), 3)
    net, args = checkpoint.load_run(root, gpu_device)
    prior = checkpoint.load_prior(root, net, args, gpu_device)  # built with the tool's 24 channels and 3 layers, not the run's flags
    assert len(prior.res_blocks) == 3 and prior.conv_in.weight.shape[0] == 24


@pytest.mark.gpu
@pytest.mark.parametrize("graph", ["off", "auto"])
def test_vis_leaves_the_trajectory_alone(gpu_device, tmp_path, graph):
    from movae_amd.visual import grid_shape

    argv = VAE + ["--epochs", "2", "--graph", graph, "--max_fid_samples", "0"]
    on, root_on, _ = _run(tmp_path / "on", argv + ["--vis", "on"])
    off, root_off, _ = _run(tmp_path / "off", argv + ["--vis", "off"])
    assert len(on) == 2 and on == off
    files = sorted(os.path.relpath(f, root_on) for f in glob.glob(os.path.join(root_on, "figures", "**", "*"), recursive=True) if os.path.isfile(f))
    assert files == sorted(os.path.join("figures", d, f"epoch_{e:04d}_{n}_samples.png") for e in (1, 2)
                           for d, n in (("generated", "random"), ("reconstructed", "test"), ("reconstructed", "train")))
    for f in files:
        want = grid_shape(4, 32, 32, 2, 2) if "random" in f else grid_shape(8, 32, 32, 4, 2)
        assert _png(os.path.join(root_on, f)).shape == (*want, 3), f
    assert not os.path.exists(os.path.join(root_off, "figures"))


@pytest.mark.gpu
def test_first_items_reads_a_resident_set_without_iterating(gpu_device):
    """The --vis pass on a device loader: rows 0 .. n-1 of the set, bit-equal to the host items, and the epoch's order untouched."""
    import movae_amd  # noqa: F401
    from movae_amd import visual
    from movae_amd.data import DeviceBatchLoader, ResidentImages

    u8 = np.random.default_rng(0).integers(0, 256, size=(10, 8, 8, 3), dtype=np.uint8)
    for train_set in (False, True):
        ds = ResidentImages(u8, normalize=True, train=train_set, seed=3)
        loader = DeviceBatchLoader(ds, 4, gpu_device, shuffle=True, seed=3)
        loader.set_epoch(2)
        ds.set_epoch(2)
        before = [b[0].clone() for b in loader]
        got = visual.first_items(loader, 3, gpu_device)
        assert got.is_cuda and torch.equal(got.cpu(), torch.stack([ds[i][0] for i in range(3)]))
        assert loader.epoch == 2 and all(torch.equal(a, b[0]) for a, b in zip(before, loader))
    assert visual.first_items(loader, 99, gpu_device).shape[0] == 10  # never more than the set holds


@pytest.mark.gpu
def test_no_figures_without_the_flag(vae_run):
    assert not os.path.exists(os.path.join(vae_run["root"], "figures"))


@pytest.mark.gpu
def test_reconstruction_grid_has_the_originals_on_top(gpu_device, vae_run, tmp_path):
    from movae_amd import checkpoint, visual

    net, _ = checkpoint.load_run(vae_run["ckpt"], gpu_device)
    path = tmp_path / "recon.png"
    originals, recons = visual.generate_reconstructed_samples(net, "test", _test_loader(gpu_device), 4, gpu_device, save_path=str(path))
    assert originals.shape == recons.shape == (4, 3, 32, 32) and originals.is_cuda and recons.is_cuda
    picture = _png(path)
    assert picture.shape == (70, 138, 3)
    both = torch.cat([originals, recons])
    lo, hi = float(both.min()), float(both.max())
    top = visual.image_grid(originals, nrow=4, normalize=True, value_range=(lo, hi), pad_value=1.0).cpu().numpy()
    bottom = visual.image_grid(recons, nrow=4, normalize=True, value_range=(lo, hi), pad_value=1.0).cpu().numpy()
    assert top.shape == (36, 138, 3) and (picture[:36] == top).all() and (picture[34:] == bottom).all()
    assert (picture[:2] == 255).all() and picture[2:34, 2:34].std() > 0

    class NoRecons(torch.nn.Module):
        def forward(self, x):
            return {"z": x}

    with pytest.raises(KeyError):
        visual.generate_reconstructed_samples(NoRecons(), "test", _test_loader(gpu_device), 4, gpu_device)

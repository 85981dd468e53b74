"""The generative evaluation (train.evaluate_generative_metrics; metrics.inception_score / kid_from_features /
precision_recall_from_features; csrc/gen_metrics.hip and the bilinear filter of csrc/inception.hip's input pipeline).

On the CPU: the loader's classifier attributes, the new flags, the host subset draw and the NaN gates.  On the GPU: every kernel
against the fixture (tests/golden/generate_gen_metrics.py, run on the CPU next to the reference: the reference's own float32 and
float64 values, the recorded KID subsets, the seeds of every input), and the stage inside train.main.

Tolerances.  A float32 quantity (prep, head, Inception Score, KID, radii) may deviate from the float64 truth by at most 4 x the
deviation of the reference's own float32 evaluation (the fixture's yardstick, or torch's float32 CPU result where the truth is
restated here), the margin test_inception_fid uses.  inception_score_from_probs sums in fp64 on both sides: 1e-12 relative.  Nearest
indices, precision and recall are exact: the generator asserts a relative margin of 1e-4 for every row of every case.  Each test
prints its figures before it asserts."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, file))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GM = _load("_gen_gen_metrics", "generate_gen_metrics.py")  # (touches the reference only inside its main())
GEN = GM.G


@pytest.fixture(scope="module")
def fx():
    return load_golden("inception_tiny")


@pytest.fixture(scope="module")
def gx():
    return load_golden("gen_metrics_tiny")


def state_dict(fx):
    return {k[3:]: torch.from_numpy(np.asarray(fx[k])).float() if k.endswith("conv.weight") else torch.from_numpy(np.asarray(fx[k]))
            for k in fx.files if k.startswith("sd.")}


@pytest.fixture
def registry(monkeypatch):
    """The module's registry, empty at the start and emptied at the end, and no environment fallback."""
    import movae_amd  # noqa: F401
    from movae_amd import inception

    monkeypatch.delenv(inception.ENV_VAR, raising=False)
    inception.use_inception_weights(None)
    yield inception
    inception.use_inception_weights(None)


@pytest.fixture
def narrow(fx, registry):
    registry.use_inception_weights(state_dict(fx))
    return registry


def within(got, truth, cpu32, what, factor=4.0):
    """max |got - truth| <= factor * max |cpu32 - truth|, printed first; -> the bound."""
    got, truth, cpu32 = (torch.as_tensor(t).detach().cpu().double() for t in (got, truth, cpu32))
    assert got.shape == truth.shape == cpu32.shape, (got.shape, truth.shape, cpu32.shape)
    err, base = (got - truth).abs().max().item(), (cpu32 - truth).abs().max().item()
    print(f"{what}: error {err:.3e}, torch fp32 CPU {base:.3e}, ratio {err / base if base else float('inf'):.2f}")
    assert math.isfinite(err) and err <= factor * base, f"{what}: {err:.3e} > {factor} x {base:.3e}"
    return factor * base


def within_yardstick(got, truth, yard, what, factor=4.0):
    got, truth = np.asarray(got, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    err = float(np.abs(got - truth).max())
    shown = f"got {got}, float64 reference {truth}, " if got.size <= 2 else f"{got.size} values, "
    print(f"{what}: {shown}error {err:.3e}, yardstick {yard:.3e}, ratio {err / yard:.2f}")
    assert math.isfinite(err) and err <= factor * yard, f"{what}: {err:.3e} > {factor} x {yard:.3e}"


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------
def test_loader_keeps_the_classifier_in_attributes(fx, registry):
    sd = state_dict(fx)
    w = registry.load_inception_weights(sd)
    assert len(w) == 3 * 94 and not any(k.startswith("fc") for k in w)
    assert w.num_classes == 10 and w.feature_dim == 256
    assert torch.equal(w.fc_weight, sd["fc.weight"].float()) and torch.equal(w.fc_bias, sd["fc.bias"].float())
    assert w.fc_weight.dtype == torch.float32 and tuple(w.fc_weight.shape) == (10, 256) and tuple(w.fc_bias.shape) == (10,)
    under = registry.load_inception_weights({"model." + k: v for k, v in sd.items()})
    assert under.num_classes == 10
    sd["AuxLogits.fc.weight"], sd["AuxLogits.fc.bias"] = torch.zeros(7, 96), torch.zeros(7)  # (stays ignored)
    assert registry.load_inception_weights(sd).num_classes == 10
    bare = registry.load_inception_weights({k: v for k, v in sd.items() if not k.startswith("fc.")})
    assert len(bare) == 3 * 94 and bare.num_classes == 0 and bare.fc_weight is None and bare.fc_bias is None


def test_loader_names_a_wrong_classifier_shape(fx, registry):
    sd = state_dict(fx)
    for key, bad in (("fc.weight", torch.zeros(10, 255)), ("fc.weight", torch.zeros(10, 256, 1)), ("fc.bias", torch.zeros(11))):
        with pytest.raises(ValueError, match=re.escape(key) + " has shape"):
            registry.load_inception_weights({**sd, key: bad})
    with pytest.raises(ValueError, match=r"fc\.bias is missing"):
        registry.load_inception_weights({k: v for k, v in sd.items() if k != "fc.bias"})


def test_parser_knows_the_stage_flags():
    import movae_amd  # noqa: F401
    from movae_amd import train

    a = train.parse_args([])
    assert a.gen_metrics == "off" and a.gen_precision_recall is False and a.max_gen_metrics_samples == 10000
    b = train.parse_args(["--gen_metrics", "on", "--gen_precision_recall", "--max_gen_metrics_samples", "96"])
    assert b.gen_metrics == "on" and b.gen_precision_recall is True and b.max_gen_metrics_samples == 96
    with pytest.raises(SystemExit):
        train.parse_args(["--gen_metrics", "maybe"])


def test_host_subset_draw_reproduces_the_recorded_indices(gx):
    import movae_amd  # noqa: F401
    from movae_amd import metrics

    ir, jf = metrics.kid_subset_indices(320, 320, 50, 50, seed=int(gx["kid.fid48.seed"]))
    assert ir.shape == (50, 50) and np.array_equal(ir, gx["kid.fid48.idx_real"]) and np.array_equal(jf, gx["kid.fid48.idx_fake"])
    rag = GM.KID_RAGGED
    ir, jf = metrics.kid_subset_indices(rag["n_real"], rag["n_fake"], rag["m"], rag["subsets"], seed=int(gx["kid.ragged.seed"]))
    assert np.array_equal(ir, gx["kid.ragged.idx_real"]) and np.array_equal(jf, gx["kid.ragged.idx_fake"])
    assert all(len(set(row)) == len(row) for row in ir)  # (without replacement)


def test_nan_gates_need_no_device(registry):
    from movae_amd import metrics

    f = torch.rand(6, 5)
    assert math.isnan(metrics.kid_from_features(f[:0], f)) and math.isnan(metrics.kid_from_features(f, f[:0]))
    assert math.isnan(metrics.kid_from_features(f[:1], f))  # m = min(50, 1, 6) < 2
    assert math.isnan(metrics.kid_from_features(f, f, subset_size=1))
    for real, fake in ((f[:0], f), (f, f[:0]), (f[:3], f), (f, f[:3])):  # empty, len <= k
        assert all(math.isnan(v) for v in metrics.precision_recall_from_features(real, fake, k=3))
    p = torch.softmax(torch.rand(7, 4), dim=1)
    assert all(math.isnan(v) for v in metrics.inception_score_from_probs(p, splits=10))  # N < splits: every split empty
    assert all(math.isnan(v) for v in metrics.inception_score_from_probs(p[:0], splits=10))
    images = torch.rand(12, 3, 32, 32)
    assert all(math.isnan(v) for v in metrics.inception_score(images[:0]))
    assert all(math.isnan(v) for v in metrics.inception_score(images[:7]))
    assert all(math.isnan(v) for v in metrics.inception_score(images))  # nothing registered


# ---- GPU: the bilinear input pipeline -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(32, 32), (40, 64)])
def test_bilinear_prep(gpu_device, h, w):
    from movae_amd import ops

    x = GEN.raw_images(700 + h + w, (2, 3, h, w), gain=1.25)
    assert x.min() < -1 and x.max() > 1  # (the clamp acts)
    truth, cpu32 = GM.bilinear_prep(x.double()), GM.bilinear_prep(x)
    got = ops.inception_prep(x.to(gpu_device), filter="bilinear")
    assert tuple(got.shape) == (2, 299, 299, 3)
    bound = within(got, truth, cpu32, f"inception_prep bilinear {h}x{w}")
    cubic = ops.inception_prep(x.to(gpu_device))
    gap = (cubic.cpu().double() - truth).abs().max().item()
    print(f"the bicubic output lies {gap:.3e} from the bilinear truth ({gap / bound:.0f} x the bound)")
    assert gap >= 10 * bound
    assert torch.equal(ops.inception_prep(x.to(gpu_device), filter="bicubic"), cubic)
    with pytest.raises(ValueError, match="filter"):
        ops.inception_prep(x.to(gpu_device), filter="nearest")
    with pytest.raises(NotImplementedError, match="299"):
        ops.inception_prep(torch.zeros((1, 3, 300, 64), device=gpu_device), filter="bilinear")


# ---- GPU: the classifier head and the Inception Score -------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n,c,d", [(37, 10, 256), (37, 13, 256), (5, 13, 50)])  # a row tail (37 = 9 x 4 + 1), a class tail, D % 4 != 0
def test_linear_softmax(fx, gpu_device, n, c, d):
    from movae_amd import ops

    g = torch.Generator().manual_seed(n * c + d)
    feat = torch.rand((n, d), generator=g) * 2.0
    weight = torch.randn((c, d), generator=g) * 0.3
    bias = torch.randn(c, generator=g)
    if (c, d) == (10, 256):
        sd = state_dict(fx)
        weight, bias = sd["fc.weight"].float() * 8.0, sd["fc.bias"].float()  # (scaled: the narrow fc alone is nearly uniform)
    truth = torch.softmax(feat.double() @ weight.double().T + bias.double(), dim=1)
    cpu32 = torch.softmax(feat @ weight.T + bias, dim=1)
    got = ops.linear_softmax(feat.to(gpu_device), weight.to(gpu_device), bias.to(gpu_device))
    assert tuple(got.shape) == (n, c) and truth.max() > 3.0 / c
    within(got, truth, cpu32, f"linear_softmax n{n} C{c} D{d}")
    assert (got.sum(1).cpu() - 1).abs().max() < 1e-5
    with pytest.raises(ValueError):
        ops.linear_softmax(feat.to(gpu_device), weight[:, :-1].contiguous().to(gpu_device), bias.to(gpu_device))


@pytest.mark.gpu
@pytest.mark.parametrize("n", GM.IS_CASES)
def test_inception_score_matches_the_reference(gx, narrow, gpu_device, n):
    from movae_amd import metrics

    x = GEN.raw_images(int(gx[f"is.{n}.seed"]), (n, 3, GM.IS_SIDE, GM.IS_SIDE)).to(gpu_device)
    got = metrics.inception_score(x)
    within_yardstick(got, gx[f"is.{n}.f64"], float(gx[f"is.{n}.yardstick"]), f"inception_score n={n}")
    probs = metrics.inception_probs(x)
    assert tuple(probs.shape) == (n, 10) and torch.equal(metrics.inception_probs(x, chunk=16), probs)
    assert metrics.inception_score_from_probs(probs) == got


@pytest.mark.gpu
def test_inception_score_gates_on_the_device(gx, narrow, gpu_device, fx):
    from movae_amd import metrics

    x = GEN.raw_images(1, (7, 3, 32, 32)).to(gpu_device)
    assert all(math.isnan(v) for v in metrics.inception_score(x))  # 7 // 10 = 0: every split empty
    assert math.isfinite(metrics.inception_score(x, splits=7)[0])
    narrow.use_inception_weights({k: v for k, v in state_dict(fx).items() if not k.startswith("fc.")})
    assert all(math.isnan(v) for v in metrics.inception_score(x, splits=7))  # no classifier
    with pytest.raises(RuntimeError, match="classifier"):
        metrics.inception_probs(x)


@pytest.mark.gpu
def test_inception_score_from_probs_is_the_float64_formula(gx, gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import metrics

    probs, ref = torch.from_numpy(gx["is.probs"]), gx["is.from_probs"]
    assert tuple(probs.shape) == (37, 13) and (probs < 1e-16).any()  # 37 // 10 = 3: seven rows dropped; the clip acts
    got = np.array(metrics.inception_score_from_probs(probs.to(gpu_device)))
    print(f"from probs {got}, float64 formula {ref}, relative {np.abs(got - ref) / ref}")
    assert np.all(np.abs(got - ref) <= 1e-12 * ref)
    one = np.array(metrics.inception_score_from_probs(probs.to(gpu_device), splits=1))  # one split of all 37 rows: std 0
    assert one[1] == 0.0 and abs(one[0] - GM.is_formula(probs.numpy(), splits=1)[0]) <= 1e-12 * one[0]


# ---- GPU: KID ---------------------------------------------------------------------------------------------------------------------
def _kid_sets(fx, gx, tag):
    if tag == "fid48":
        return fx["fid.features"][0], fx["fid.features"][1]
    rag = GM.KID_RAGGED
    return GM.kid_ragged_sets(int(gx["kid.ragged.set_seed"]), rag["n_real"], rag["n_fake"], rag["dim"])


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["fid48", "ragged"])
def test_kid_matches_the_reference(fx, gx, gpu_device, tag):
    import movae_amd  # noqa: F401
    from movae_amd import metrics

    real, fake = (torch.from_numpy(np.ascontiguousarray(t)).to(gpu_device) for t in _kid_sets(fx, gx, tag))
    subsets = (gx[f"kid.{tag}.idx_real"], gx[f"kid.{tag}.idx_fake"])
    kw = dict(degree=int(gx[f"kid.{tag}.degree"]), gamma=float(gx[f"kid.{tag}.gamma"])) if tag == "ragged" else {}
    got = metrics.kid_from_features(real, fake, subsets=subsets, **kw)
    within_yardstick(got, float(gx[f"kid.{tag}.f64"]), float(gx[f"kid.{tag}.yardstick"]), f"kid {tag}")
    # the host draw from the recorded seed gives the same subsets, hence the same bits
    m, s = subsets[0].shape[1], subsets[0].shape[0]
    assert metrics.kid_from_features(real, fake, subset_size=m, n_subsets=s, seed=int(gx[f"kid.{tag}.seed"]), **kw) == got
    with pytest.raises(ValueError, match="outside"):
        metrics.kid_from_features(real, fake, subsets=(subsets[0] + real.size(0), subsets[1]), **kw)


# ---- GPU: nearest neighbours, precision and recall ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tile", [64, 128, None])
@pytest.mark.parametrize("tag", [t for t, _, _ in GM.PR_CASES])
def test_knn_rows_matches_the_reference(gx, gpu_device, tag, tile):
    from movae_amd import ops

    na, nb, dim = (int(v) for v in gx[f"pr.{tag}.shape"])
    k, yard = int(gx[f"pr.{tag}.k"]), float(gx[f"pr.{tag}.yardstick"])
    real, fake = (torch.from_numpy(t).to(gpu_device) for t in GM.knn_sets(int(gx[f"pr.{tag}.seed"]), na, nb, dim))
    for what, s, key in (("real/real", real, "radius_real"), ("fake/fake", fake, "radius_fake")):
        d2, _ = ops.knn_rows(s, s, k, exclude_diag=True, tile=tile)
        assert tuple(d2.shape) == (s.size(0), k) and (d2[:, 1:] >= d2[:, :-1]).all() and (d2 >= 0).all()
        within_yardstick(d2[:, k - 1].sqrt().cpu().numpy(), gx[f"pr.{tag}.{key}"], yard, f"knn_rows {tag} tile {tile} {what} radius")
    for what, q, s, key in (("fake->real", fake, real, "nn_fake_to_real"), ("real->fake", real, fake, "nn_real_to_fake")):
        d2, idx = ops.knn_rows(q, s, 1, tile=tile)
        wrong = int((idx.cpu().numpy() != gx[f"pr.{tag}.{key}"]).sum())
        print(f"knn_rows {tag} tile {tile} {what}: {wrong} of {idx.numel()} nearest indices differ")
        assert idx.dtype == torch.int32 and wrong == 0
        exact = (q.double() - s.double()[idx.long()]).pow(2).sum(1).sqrt().cpu().numpy()
        within_yardstick(d2[:, 0].sqrt().cpu().numpy(), exact, yard, f"knn_rows {tag} tile {tile} {what} distance")
    without, _ = ops.knn_rows(real, real, 1, tile=tile)  # the diagonal kept: every row finds itself
    # (|a|^2 <= 4 D = 200, summed over D = 50 fp32 products: the Gram form of a row with itself errs by less than 200 x 50 x 2^-24)
    assert without.max().item() <= 1e-3 and ops.knn_rows(real, real, 1, exclude_diag=True, tile=tile)[0].min().item() > 0.01


@pytest.mark.gpu
@pytest.mark.parametrize("tag", [t for t, _, _ in GM.PR_CASES])
def test_precision_recall_are_the_references(gx, gpu_device, tag):
    import movae_amd  # noqa: F401
    from movae_amd import metrics

    na, nb, dim = (int(v) for v in gx[f"pr.{tag}.shape"])
    real, fake = (torch.from_numpy(t).to(gpu_device) for t in GM.knn_sets(int(gx[f"pr.{tag}.seed"]), na, nb, dim))
    got = metrics.precision_recall_from_features(real, fake, k=int(gx[f"pr.{tag}.k"]))
    ref = (float(gx[f"pr.{tag}.precision"]), float(gx[f"pr.{tag}.recall"]))
    print(f"precision / recall {tag}: {got}, reference {ref}")
    # fractions of nb and na rows: float32 means of 0 / 1 values against the reference's float64 means
    assert round(got[0] * nb) == round(ref[0] * nb) and round(got[1] * na) == round(ref[1] * na)
    assert abs(got[0] - ref[0]) <= 1e-6 and abs(got[1] - ref[1]) <= 1e-6


@pytest.mark.gpu
def test_knn_rows_refusals(gpu_device):
    from movae_amd import ops

    a = torch.rand(6, 5, device=gpu_device)
    with pytest.raises(ValueError, match="k must be"):
        ops.knn_rows(a, a, 9)
    with pytest.raises(ValueError, match="k must be"):
        ops.knn_rows(a, a, 6, exclude_diag=True)  # five candidates per row
    with pytest.raises(ValueError, match="tile"):
        ops.knn_rows(a, a, 1, tile=32)
    with pytest.raises(ValueError, match="do not match"):
        ops.knn_rows(a, a[:, :4].contiguous(), 1)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.knn_rows(a.cpu(), a.cpu(), 1)


# ---- GPU: the stage -----------------------------------------------------------------------------------------------------------------
VAE_ARGV = ["--dataset", "synthetic_cifar10", "--arch", "vae", "--agg", "upgrad", "--batch_size", "50", "--max_items", "1000", "--latent_dim",
            "16", "--hidden_dims", "16", "32", "--seed", "2", "--device", "cuda:0", "--graph", "off", "--epochs", "1", "--eval_freq", "0",
            "--max_fid_samples", "0", "--max_gen_metrics_samples", "96"]
ORDER = ("gfid", "inception_score_mean", "inception_score_std", "kid", "precision", "recall")


def _run(train, argv, tmp_path, capsys):
    args = train.parse_args(argv + ["--save_path", str(tmp_path)])
    train.set_seed(args.seed)
    train.main(args)
    return [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("generative: ")]


@pytest.mark.gpu
def test_training_run_reports_the_generative_metrics(narrow, gpu_device, tmp_path, capsys, monkeypatch):
    from movae_amd import metrics, train

    lines = _run(train, VAE_ARGV + ["--gen_metrics", "on", "--gen_precision_recall"], tmp_path, capsys)
    assert len(lines) == 1
    gen = train.LAST_FINAL["gen"]
    print("reported " + lines[0])  # (prefixed: the next run's capture must not find it again)
    assert tuple(sorted(gen)) == tuple(sorted(ORDER)) and all(math.isfinite(v) for v in gen.values()), gen
    found = re.findall(r"(\w+): ([-+0-9.eE]+|nan|inf)", lines[0][len("generative: "):])
    assert [k for k, _ in found] == list(ORDER)
    for k, v in found:
        assert float(v) == pytest.approx(gen[k], abs=1e-5), k
    last = train.LAST_GEN
    assert last["n"] == 96 and tuple(last["real_features"].shape) == tuple(last["fake_features"].shape) == (96, 256)
    assert tuple(last["probs"].shape) == (96, 10)
    assert gen["gfid"] == metrics.fid_from_features(last["real_features"], last["fake_features"]) and gen["gfid"] > 0
    assert gen["kid"] == metrics.kid_from_features(last["real_features"], last["fake_features"], seed=2)
    assert (gen["inception_score_mean"], gen["inception_score_std"]) == metrics.inception_score_from_probs(last["probs"])
    assert 0.0 <= gen["precision"] <= 1.0 and 0.0 <= gen["recall"] <= 1.0 and gen["inception_score_mean"] >= 1.0
    # without --gen_precision_recall the two stay NaN (the reference's present behaviour); without fc, IS alone is NaN
    lines = _run(train, VAE_ARGV + ["--gen_metrics", "on"], tmp_path, capsys)
    gen = train.LAST_FINAL["gen"]
    assert len(lines) == 1 and math.isnan(gen["precision"]) and math.isnan(gen["recall"]) and math.isfinite(gen["kid"])
    assert re.search(r"precision: nan, recall: nan$", lines[0])


@pytest.mark.gpu
def test_stage_is_off_by_default(narrow, gpu_device, tmp_path, capsys, monkeypatch):
    from movae_amd import train

    monkeypatch.setattr(train, "evaluate_generative_metrics", lambda *a, **k: pytest.fail("the stage ran with --gen_metrics off"))
    assert _run(train, VAE_ARGV + ["--gen_metrics", "off"], tmp_path, capsys) == [] and "gen" not in train.LAST_FINAL
    assert _run(train, VAE_ARGV, tmp_path, capsys) == [] and "gen" not in train.LAST_FINAL


@pytest.mark.gpu
def test_stage_without_weights_generates_nothing(registry, gpu_device, tmp_path, capsys, monkeypatch):
    from movae_amd import train
    from movae_amd.models import vae

    monkeypatch.setattr(vae.VAE, "sample", lambda *a, **k: pytest.fail("generated without Inception weights"))
    lines = _run(train, VAE_ARGV + ["--gen_metrics", "on", "--gen_precision_recall"], tmp_path, capsys)
    gen = train.LAST_FINAL["gen"]
    assert len(lines) == 1 and sorted(gen) == sorted(ORDER) and all(math.isnan(v) for v in gen.values())
    assert train.LAST_GEN == {}


@pytest.mark.gpu
def test_the_prior_reaches_the_stage(narrow, gpu_device, tmp_path, capsys, monkeypatch):
    from movae_amd import prior as P
    from movae_amd import train

    calls = []
    real_generate = P.generate_samples_vq_with_prior

    def recording(net, prior, num_samples, device, temperature=1.0, cached=False):
        calls.append((prior, num_samples, temperature, cached))
        return real_generate(net, prior, num_samples, device, temperature, cached=cached)

    monkeypatch.setattr(P, "generate_samples_vq_with_prior", recording)
    argv = ["--dataset", "synthetic_cifar10", "--arch", "vq_vae", "--embedding_dim", "8", "--num_embeddings", "16", "--hidden_dims", "16",
            "32", "--batch_size", "16", "--max_items", "512", "--epochs", "1", "--pixelcnn_epochs", "1", "--pixelcnn_hidden_channels", "16",
            "--pixelcnn_num_layers", "2", "--pixelcnn_lr", "3e-3", "--seed", "1", "--device", "cuda:0", "--eval_freq", "0",
            "--max_fid_samples", "0", "--prior_sampler", "cached", "--pixelcnn_temperature", "0.9", "--num_vis_samples", "3",
            "--gen_metrics", "on", "--max_gen_metrics_samples", "32"]
    lines = _run(train, argv, tmp_path, capsys)
    gen = train.LAST_FINAL["gen"]
    assert len(lines) == 1 and math.isfinite(gen["gfid"]) and math.isfinite(gen["kid"]) and math.isfinite(gen["inception_score_mean"])
    stage = [c for c in calls if c[1] != 3]  # (the prior stage draws its --num_vis_samples itself)
    assert [c[1] for c in stage] == [16, 16] and len(calls) == 3
    assert all(c[0] is P.LAST_RUN["prior"] and c[2] == 0.9 and c[3] is True for c in calls)
    assert train.LAST_GEN["n"] == 32

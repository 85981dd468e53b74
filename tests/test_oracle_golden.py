"""Pins the CPU oracle (oracle/) against golden vectors generated from the reference's own code
(tests/golden/generate_golden.py).  CPU only."""
import numpy as np
import pytest
import torch

from conftest import cfg_from_meta, load_golden, meta_of
from oracle import aggregation as A
from oracle import nets, objectives as O
from oracle.step import OracleTrainer

TINY = ["vae_tiny", "vae_tiny_bce", "vae_1x1", "vq_vae_tiny", "vq_vae2_tiny", "betatc_vae_tiny", "gg_vae_tiny", "gg_vq_vae_tiny", "gg_vq_vae2_tiny",
        "gg_vq_vae_v4_tiny", "gg_vae_v5_tiny"]


def T(a):
    return torch.from_numpy(np.asarray(a))


# ---------------------------------------------------------------- objectives
@pytest.mark.parametrize("name,fn,rkey", [("mse", O.mse, "r_tanh"), ("l1", O.l1, "r_tanh"),
                                          ("smooth_l1", O.smooth_l1, "r_sl1"), ("bce", O.bce, "r_sig")])
def test_objective_values_and_grads(name, fn, rkey):
    fx = load_golden("objectives")
    x, r = T(fx["x"]), T(fx[rkey]).requires_grad_(True)
    v = fn(x, r)
    (g,) = torch.autograd.grad(v, r)
    np.testing.assert_allclose(v.item(), fx[f"{name}.value"], rtol=2e-6)
    # bce: the reference's ATen kernel clamps the gradient denominator; skip the two saturated points
    gg, ge = g.numpy().reshape(-1), fx[f"{name}.grad"].reshape(-1)
    sl = slice(2, None) if name == "bce" else slice(None)
    np.testing.assert_allclose(gg[sl], ge[sl], rtol=1e-5, atol=1e-9)


def test_kl():
    fx = load_golden("objectives")
    mu, lv = T(fx["kl.mu"]).requires_grad_(True), T(fx["kl.log_var"]).requires_grad_(True)
    v = O.kl_divergence(mu, lv)
    gm, gl = torch.autograd.grad(v, [mu, lv])
    np.testing.assert_allclose(v.item(), fx["kl.value"], rtol=1e-6)
    np.testing.assert_allclose(gm.numpy(), fx["kl.gmu"], rtol=1e-6, atol=1e-9)
    # d/dlv = (e^lv - 1) / 2B is formed as 0.5/B * e^lv - 0.5/B, which cancels near lv = 0: there its last place is that of the
    # term 0.5/B * e^lv (7.5e-9 at lv = 0.04, B = 5), and exp may return either neighbour of a value near a rounding midpoint
    # (MKL's AVX-512 and AVX2 paths do, at lv = 0.0413).  So each element may be one place of that term off the reference's.
    term = (0.5 / fx["kl.mu"].shape[0] * np.exp(fx["kl.log_var"].astype(np.float64))).astype(np.float32)
    err = np.abs(gl.numpy() - fx["kl.glv"]) - (1e-6 * np.abs(fx["kl.glv"]) + 1e-9 + np.spacing(term))
    assert err.max() <= 0, f"d kl / d log_var off by more than one place of the e^lv term: {np.argwhere(err > 0).tolist()}"


def test_activation_table():
    fx = load_golden("objectives")
    for s in fx["activation_table"]:
        key, want = str(s).split("=")
        obj, act = key.split("|")
        _, got = O.resolve_objective(obj, None if act == "None" else act)
        assert got == want, key


# ---------------------------------------------------------------- weightings
CASES = ["kat", "k2", "k3", "k3_zero_row", "k4", "k4_conflict", "k5_rankdef", "k2_parallel"]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("nt", ["none", "l2", "loss", "loss+"])
def test_mgda_weights(case, nt):
    fx = load_golden("weightings")
    w, it = A.mgda_weights(fx[f"{case}.G"], nt, fx[f"{case}.losses"], return_iters=True)
    np.testing.assert_allclose(w, fx[f"{case}.mgda.{nt}"], rtol=2e-4, atol=2e-6)


@pytest.mark.parametrize("case", CASES)
def test_stable_mgda_weights(case):
    """StableMGDA's eigen regularisation (utils/torchmoo/mgda.py:286-317) against the reference's own weights."""
    fx = load_golden("weightings")
    np.testing.assert_allclose(A.mgda_weights(fx[f"{case}.G"], "none", stable=True), fx[f"{case}.mgda.stable"], rtol=5e-4, atol=5e-6)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("sm", ["min", "median", "rmse"])
def test_aligned_mtl_weights(case, sm):
    fx = load_golden("weightings")
    G = fx[f"{case}.G"]
    w = A.aligned_mtl_weights(G, sm)
    want = fx[f"{case}.amtl.{sm}"]
    # near-singular Gramians amplify eigh rounding by 1/sqrt(lambda_min); compare through G
    np.testing.assert_allclose(w, want, rtol=5e-3, atol=1e-5 * np.abs(want).max())


def test_mgda_docstring_kats():
    """utils/torchmoo/mgda.py:54-86."""
    J = torch.tensor([[-4.0, 1.0, 1.0], [6.0, 1.0, 1.0]])
    want = {"none": [0.0, 1.0, 1.0], "l2": [1.0, 1.0, 1.0], "loss": [3.49, 1.0, 1.0], "loss+": [4.1606, 1.0, 1.0]}
    fx = load_golden("weightings")
    for nt, exp in want.items():
        w = A.mgda_weights((J @ J.T).numpy(), nt, np.array([0.5, 2.0], dtype=np.float32))
        g = torch.as_tensor(w) @ J
        np.testing.assert_allclose(g.numpy(), fx[f"kat.mgda_agg.{nt}"], rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(g.numpy(), exp, atol=5e-4)


def test_upgrad_docstring_kat():
    """utils/torchmoo/nupgrad.py:58-62 (torchjd's UPGrad example)."""
    J = torch.tensor([[-4.0, 1.0, 1.0], [6.0, 1.0, 1.0]])
    w = A.upgrad_weights(J @ J.T)
    np.testing.assert_allclose(w, [1.11092105, 0.78943103], rtol=1e-6)
    np.testing.assert_allclose((torch.as_tensor(w, dtype=torch.float32) @ J).numpy(), [0.2929, 1.9004, 1.9004], atol=5e-5)


@pytest.mark.parametrize("case", CASES)
def test_upgrad_against_scipy(case):
    """Independent check of the active-set enumeration with a generic constrained solver."""
    from scipy.optimize import minimize

    fx = load_golden("weightings")
    G = fx[f"{case}.G"].astype(np.float64)
    K = len(G)
    tr = np.trace(G)
    Gn = (G / tr if tr >= 1e-4 else np.zeros_like(G)) + 1e-4 * np.eye(K)
    total = np.zeros(K)
    for i in range(K):
        u = np.zeros(K)
        u[i] = 1.0 / K
        r = minimize(lambda w: 0.5 * w @ Gn @ w, u + 0.1, jac=lambda w: Gn @ w, method="SLSQP",
                     bounds=[(u[j], None) for j in range(K)], options=dict(ftol=1e-15, maxiter=500))
        total += r.x
    np.testing.assert_allclose(A.upgrad_weights(fx[f"{case}.G"]), total, rtol=2e-4, atol=2e-5)


def test_nupgrad_pnupgrad_normalisations_and_comfort_schedule_match_reference_code():
    """the in-tree pieces of NUPGrad / PNUPGrad / COMFORT against vectors generated from
    utils/torchmoo/{nupgrad,pnupgrad,comfort}.py (tests/golden/agg_variants.npz).  The projection itself is torchjd's."""
    fx, wx = load_golden("agg_variants"), load_golden("weightings")
    for name in fx["cases"]:
        G = wx[f"{name}.G"]
        for eps in (1e-4, 1e-2):
            np.testing.assert_allclose(A.normalize_min_l2(G, eps), fx[f"{name}.min_l2.{eps}"], rtol=1e-6, atol=1e-7)
            np.testing.assert_array_equal(fx[f"{name}.min_l2.{eps}"], fx[f"{name}.min_l2_p.{eps}"])  # the two in-tree copies agree
            np.testing.assert_allclose(A.normalize_cosine(G, eps), fx[f"{name}.cosine.{eps}"], rtol=1e-6, atol=1e-7)
            np.testing.assert_allclose(A.normalize_min_l2(G, eps) + eps * np.eye(len(G), dtype=np.float32), fx[f"{name}.reg.{eps}"],
                                       rtol=1e-6, atol=1e-7)
    assert not A.normalize_min_l2(np.zeros((3, 3), np.float32), 1e-4).any() and not fx["zero.min_l2"].any()
    for e, t, k, a, l, u, b in fx["beta_schedule"]:
        assert abs(A.beta_schedule(int(e), int(t), k, a, l, u) - b) < 1e-12


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("norm", ["min_l2", "cosine"])
def test_nupgrad_projection_against_scipy(case, norm):
    """Independent check of the projection on the NUPGrad / PNUPGrad Gramians with a generic constrained solver."""
    from scipy.optimize import minimize

    fx = load_golden("weightings")
    G = fx[f"{case}.G"]
    K = len(G)
    Gn = (A.normalize_min_l2(G, 1e-4) if norm == "min_l2" else A.normalize_cosine(G, 1e-4)).astype(np.float64) + 1e-4 * np.eye(K)
    total = np.zeros(K)
    for i in range(K):
        u = np.zeros(K)
        u[i] = 1.0 / K
        r = minimize(lambda w: 0.5 * w @ Gn @ w, u + 0.1, jac=lambda w: Gn @ w, method="SLSQP",
                     bounds=[(u[j], None) for j in range(K)], options=dict(ftol=1e-15, maxiter=500))
        total += r.x
    np.testing.assert_allclose(A.upgrad_weights(G, norm=norm), total, rtol=5e-4, atol=5e-5)


# ---------------------------------------------------------------- models
def _trainer(fx, agg="sum"):
    m = meta_of(fx)
    cfg = nets.make_cfg(**cfg_from_meta(m))
    tr = OracleTrainer(cfg, seed=int(m["seed"]), agg=agg)
    return tr, m


@pytest.mark.parametrize("tag", TINY)
def test_init_replays_reference_constructor(tag):
    fx = load_golden(tag)
    tr, _ = _trainer(fx)
    keys = [k[4:] for k in fx.files if k.startswith("sd0.")]
    assert list(tr.sd.keys()) == keys
    for k in keys:
        assert np.array_equal(tr.sd[k].detach().numpy(), fx["sd0." + k]), k


@pytest.mark.parametrize("tag", TINY)
def test_forward_losses_grads_and_adam_step(tag):
    fx = load_golden(tag)
    tr, m = _trainer(fx)
    x = T(fx["x"])
    eps = T(fx["eps.0"]) if "eps.0" in fx.files else None
    out, ld, grads, _ = tr.grads(x, eps)
    for k in [f[4:] for f in fx.files if f.startswith("out.")]:
        got = out[k]
        got = got.detach().numpy() if isinstance(got, torch.Tensor) else np.array(got)
        if got.dtype.kind in "iu":
            assert np.array_equal(got, fx["out." + k]), k
        else:
            np.testing.assert_allclose(got, fx["out." + k], rtol=2e-5, atol=2e-6, err_msg=k)
    assert list(ld.keys()) == [f[5:] for f in fx.files if f.startswith("loss.")]
    for k, v in ld.items():
        np.testing.assert_allclose(v.item(), fx["loss." + k], rtol=1e-5, atol=1e-7, err_msg=k)
    for n, g in grads.items():
        want = fx["gsum." + n]
        np.testing.assert_allclose(g.numpy(), want, rtol=1e-3, atol=2e-6 * max(1.0, np.abs(want).max()), err_msg=n)
    # Adam step + BN running statistics.  The step is taken on the reference's own gradients (the oracle's are held to them
    # just above): Adam's first step lr * g / (|g| + eps) magnifies a rounding-level difference in a gradient near eps (1e-8)
    # some 3e4-fold, so the oracle's gradients would carry the BLAS rounding of the host's CPU (MKL's AVX-512 and AVX2 paths
    # round differently) into the small-gradient weights
    for n, p in tr.params.items():
        p.grad = T(fx["gsum." + n]).clone()
    tr.opt.step()
    for k in tr.sd:
        want = fx["sd1." + k]
        got = tr.sd[k].detach().numpy()
        if k.endswith("num_batches_tracked"):
            assert got == want
        else:
            # a conv bias in front of BatchNorm has an analytically zero gradient; the reference's
            # own value is ~1e-9 rounding noise which Adam turns into a +-lr step (ill-defined).
            noise = ("gsum." + k) in fx.files and np.abs(fx["gsum." + k]).max() < 1e-6
            np.testing.assert_allclose(got, want, rtol=1e-4, atol=2.1e-3 if noise else 2e-5, err_msg=k)
    # second step on the same batch (running stats / anneal counter advance exactly once per step)
    _, ld2 = tr.forward(x, eps)
    for k, v in ld2.items():
        np.testing.assert_allclose(v.item(), fx["loss2." + k], rtol=5e-4, atol=1e-6, err_msg=k)


@pytest.mark.parametrize("tag", TINY)
def test_per_loss_gradients_and_feature_gradients(tag):
    fx = load_golden(tag)
    tr, m = _trainer(fx)
    x = T(fx["x"])
    eps = T(fx["eps.0"]) if "eps.0" in fx.files else None
    out, ld = tr.forward(x, eps)
    comp = [v for k, v in ld.items() if k != "total_loss"]
    feats = [out[f] for f in tr.arch["features"]]
    ps = list(tr.params.values())
    for i, l in enumerate(comp):
        gs = torch.autograd.grad(l, ps + feats, retain_graph=True, allow_unused=True)
        for n, p, g in zip(tr.params, ps, gs):
            want = fx[f"gloss.{i}.{n}"]
            got = np.zeros_like(want) if g is None else g.numpy()
            np.testing.assert_allclose(got, want, rtol=1e-3, atol=2e-6 * max(1.0, np.abs(want).max()), err_msg=f"{i}.{n}")
        for f, g in zip(tr.arch["features"], gs[len(ps):]):
            want = fx[f"gfeat.{i}.{f}"]
            got = np.zeros_like(want) if g is None else g.numpy()
            np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-6 * max(1.0, np.abs(want).max()), err_msg=f)


@pytest.mark.parametrize("tag", ["vae_tiny", "vq_vae_tiny", "betatc_vae_tiny"])
def test_mtl_backward_rows_equal_reference_per_loss_gradients(tag):
    """For non-nested features J[i] restricted to the shared parameters equals d loss_i / d theta
    taken by plain autograd on the reference model, and unit weights reproduce total.backward()."""
    from oracle import autojac

    fx = load_golden(tag)
    tr, m = _trainer(fx, agg="jd_sum")
    x = T(fx["x"])
    eps = T(fx["eps.0"]) if "eps.0" in fx.files else None
    out, ld = tr.forward(x, eps)
    comp = [v for k, v in ld.items() if k != "total_loss"]
    feats = [out[f] for f in tr.arch["features"]]
    J, shared, task = autojac.jacobian_mtl(tr.params, comp, feats)
    for i in range(len(comp)):
        want = np.concatenate([fx[f"gloss.{i}.{n}"].reshape(-1) for n in shared])
        np.testing.assert_allclose(J[i].numpy(), want, rtol=1e-3, atol=2e-6 * max(1.0, np.abs(want).max()))
    grads, info = autojac.mtl_backward(tr.params, comp, feats, A.make_weighting("jd_sum"))
    for n, g in grads.items():
        want = fx["gsum." + n]
        np.testing.assert_allclose(g.numpy(), want, rtol=1e-3, atol=3e-6 * max(1.0, np.abs(want).max()), err_msg=n)
    assert set(shared).isdisjoint(task.keys())
    assert set(shared) | set(task.keys()) == set(tr.params.keys())


@pytest.mark.parametrize("tag", ["vae_tiny", "vq_vae_tiny", "betatc_vae_tiny", "vq_vae2_tiny"])
@pytest.mark.parametrize("agg", ["mgda", "mgda_ln", "mgda_gn", "mgda_lgn", "aligned_mtl", "aligned_mtl_rmse"])
def test_weightings_on_model_gramians_match_reference_code(tag, agg):
    """Weights for the model's own Gramian were produced by the reference's weighting classes at
    fixture time only for the standalone cases; here the oracle's weighting must at least give a
    finite, K-long vector and the combine must stay finite (reference behaviour incl. zero rows)."""
    if tag == "betatc_vae_tiny" and agg in ("mgda_gn", "mgda_lgn"):
        pytest.skip("negative tc_loss is clamped to 1e-20 by the reference (mgda.py:334) -> inf/NaN there too")
    fx = load_golden(tag)
    tr, m = _trainer(fx, agg=agg)
    x = T(fx["x"])
    eps = T(fx["eps.0"]) if "eps.0" in fx.files else None
    out, ld, grads, info = tr.grads(x, eps)
    assert info["w"].shape[0] == len(ld) - 1
    assert torch.isfinite(info["w"]).all()
    for g in grads.values():
        assert torch.isfinite(g).all()


def test_full_size_step0_scalars():
    """C1/C2 (CIFAR VAE) step-0 losses at BASELINE.json's sizes; the larger configs are covered on
    the GPU box by the HIP-vs-fixture test."""
    fx = load_golden("full_configs")
    for tag in ["C1", "C2"]:
        m = {}
        for s in fx[f"{tag}.meta"]:
            k, v = str(s).split("=", 1)
            m[k] = v
        m["objective"] = "mse"
        cfg = nets.make_cfg(**cfg_from_meta(m))
        seed = int(m["seed"])
        tr = OracleTrainer(cfg, seed=seed)
        x = torch.rand(int(m["B"]), 3, 32, 32, generator=torch.Generator().manual_seed(seed + 1))
        eps = torch.randn(int(m["B"]), cfg["latent_dim"], generator=torch.Generator().manual_seed(seed + 2))
        out, ld, grads, _ = tr.grads(x, eps)
        for k, v in ld.items():
            np.testing.assert_allclose(v.item(), fx[f"{tag}.loss.{k}"], rtol=1e-5, err_msg=k)
        for n, g in grads.items():
            s, l2 = fx[f"{tag}.g.{n}"]
            np.testing.assert_allclose(g.double().norm().item(), l2, rtol=1e-3, atol=1e-6, err_msg=n)


EDGE_MODES = ["mag", "signed_mse", "maxnorm", "angle", "masked", "cosine"]


@pytest.mark.parametrize("case", ["rand", "far", "flat"])
def test_edge_matching_variants_match_reference_methods(case):
    """oracle.nets.edge_matching_variant vs the reference's GGVQVAE.edge_matching_loss_v1..v6 and GGVAE.edge_matching_loss
    [_v2/_v3/_v5] (tests/golden/edge_variants.npz): loss and gradient w.r.t. the reconstruction."""
    fx = load_golden("edge_variants")
    x, r = torch.from_numpy(fx["x"]), torch.from_numpy(fx[f"{case}.recons"])
    seen = 0
    for mode in EDGE_MODES:
        for prefix in ("", "gg_vae."):
            key = f"{case}.{prefix}{mode}"
            if key + ".loss" not in fx.files:
                continue
            rr = r.clone().requires_grad_(True)
            loss = nets.edge_matching_variant(x, rr, mode)
            (g,) = torch.autograd.grad(loss, rr)
            np.testing.assert_allclose(loss.item(), fx[key + ".loss"], rtol=1e-6, err_msg=key)
            np.testing.assert_allclose(g.numpy(), fx[key + ".grad"], rtol=1e-5, atol=1e-9, err_msg=key)
            seen += 1
    assert seen >= (6 if case == "flat" else 10)


def test_torchjd_dualproj_pcgrad_imtlg_cagrad_usage_examples():
    """torchjd's documented usage example J = [[-4, 1, 1], [6, 1, 1]] (the same matrix utils/torchmoo/mgda.py:54-86 and
    nupgrad.py:58-62 quote for MGDA / UPGrad): DualProj -> [0.5563, 1.1109, 1.1109], PCGrad -> [0.5848, 3.8012, 3.8012],
    IMTLG -> [0.0767, 1.0000, 1.0000].  The only published vectors for these three (torchjd is absent): parity unpinned
    beyond them."""
    from oracle import aggregation as OA

    J = torch.tensor([[-4.0, 1.0, 1.0], [6.0, 1.0, 1.0]])
    G = (J @ J.T).numpy()
    for w, want in ((OA.dualproj_weights(G), [0.5563, 1.1109, 1.1109]), (OA.pcgrad_weights(G), [0.5848, 3.8012, 3.8012]),
                    (OA.imtlg_weights(G), [0.0767, 1.0, 1.0])):
        np.testing.assert_allclose((torch.as_tensor(w, dtype=torch.float32) @ J).numpy(), want, atol=5e-5)
    # CAGrad(c=0.5) on the same matrix: torchjd documents [0.1835, 1.2041, 1.2041]
    np.testing.assert_allclose((torch.as_tensor(OA.cagrad_weights(G, 0.5), dtype=torch.float32) @ J).numpy(), [0.1835, 1.2041, 1.2041],
                               atol=5e-5)
    np.testing.assert_allclose(OA.cagrad_weights(np.zeros((3, 3)), 1.0), np.full(3, 1 / 3))  # c g0 <= norm_eps: mean weights
    # DualProj = the single-row case of the UPGrad projection; K = 1 degenerates to the mean weight
    np.testing.assert_allclose(OA.dualproj_weights(np.array([[2.0]])), [1.0])
    np.testing.assert_allclose(OA.imtlg_weights(np.zeros((3, 3))), np.zeros(3))

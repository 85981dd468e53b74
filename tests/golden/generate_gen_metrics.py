#!/usr/bin/env python3
"""Golden vectors of the generative evaluation -- Inception Score, KID, precision / recall (runs ONLY in the build container, on the
CPU, never on the GPU box).

Imports generate_inception.py (the narrow Inception-v3, its seeded weights -- those of inception_tiny.npz, `fc` of 10 classes
included -- the image generators and the torchvision stub) and the reference's utils/metrics.py by path, and lets the reference's
calculate_inception_score / kid_from_features / precision_recall_from_features run unmodified.  Two additions to the stub:

  * the narrow module gets a `forward` (stem, blocks, global average pool, eval-mode dropout = the identity, `fc`), STATED FROM
    KNOWLEDGE of torchvision's public definition like the rest of that file;
  * `resize` also accepts TF.resize's default filter, BILINEAR, on F.interpolate(mode="bilinear", antialias=True).

For KID numpy.random.default_rng is replaced by a seeded generator that records what it draws.

  gen_metrics_tiny.npz
    is.<n>.{seed,ref,f64,f32_cl,yardstick}   calculate_inception_score of raw_images(seed, (n, 3, 32, 32)), n = 40 and 37: (mean, std)
                                             of the reference in float32, of a float64 copy of everything, and of a second float32 run
                                             in channels_last memory; yardstick = max |fp32 - f64| over both runs and both numbers
    is.probs, is.from_probs                  [37, 13] float32 probabilities with entries below 1e-16 (seeded, peaky) and the
                                             reference's formula on them in float64: (mean, std)
    kid.<tag>.{seed,idx_real,idx_fake,gamma,degree,ref,f64,f32_perm,yardstick}
                                             tag "fid48": the two [320, 48] feature sets of inception_tiny.npz, m = 50, S = 50, the
                                             defaults; tag "ragged": seeded [23, 50] / [19, 50] sets of ONE distribution (some subsets'
                                             MMD^2 is negative: the clamp acts), m = 7, S = 3, degree 3, gamma 0.03.  ref: the reference
                                             on the float32 features; f64: on their float64 copies; f32_perm: float32 with the feature
                                             columns permuted (another accumulation order)
    pr.<tag>.{seed,shape,k,radius_real,radius_fake,nn_fake_to_real,nn_real_to_fake,precision,recall,yardstick}
                                             knn_sets(seed, na, nb, D): `real` [na, D], `fake` [nb, D]; the k-th neighbour radii of both
                                             sets and the nearest indices in float64, the reference's precision / recall, and
                                             yardstick = max |float32 numpy Gram-form radius - float64 radius|

Asserted here: every recorded row of every pr case has a relative margin of at least 1e-4 both between its nearest distance and the
radius it is compared with and between its nearest and second nearest distance (the seeds are searched until that holds), so a correct
fp32 implementation reproduces the indices and the two fractions exactly; and plausible wrong variants -- bicubic instead of bilinear
for IS, no clip, the split remainder kept, the KID diagonals kept, divisor m^2, no clamp at 0, P/R without the diagonal exclusion, the
radius at k + 1 -- differ from the reference by more than 10 times the GPU test's bound (4 x yardstick; any difference for the exact
P/R fractions).

Usage:  python tests/golden/generate_gen_metrics.py        (about a minute)
"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "gen_metrics_tiny.npz")


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, file))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load("_gen_inception", "generate_inception.py")
SEED = G.SEED + 500
IS_CASES = (40, 37)
IS_SIDE = 32
KID_RAGGED = dict(n_real=23, n_fake=19, dim=50, m=7, subsets=3, degree=3, gamma=0.03)
PR_CASES = (("130x97x50k3", (130, 97, 50), 3), ("130x97x50k5", (130, 97, 50), 5), ("64x64x8k3", (64, 64, 8), 3))
MARGIN = 1e-4
#: the filter the stub's resize uses when the caller names none; "bicubic" is the WRONG pipeline of the negative check
RESIZE = {"default": "bilinear"}


# ---- additions to generate_inception's stub ------------------------------------------------------------------------------------------
def narrow_forward(self, x):
    x = self.Conv2d_2b_3x3(self.Conv2d_2a_3x3(self.Conv2d_1a_3x3(x)))
    x = F.max_pool2d(x, kernel_size=3, stride=2)
    x = self.Conv2d_4a_3x3(self.Conv2d_3b_1x1(x))
    x = F.max_pool2d(x, kernel_size=3, stride=2)
    for name in ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7a", "Mixed_7b",
                 "Mixed_7c"):
        x = getattr(self, name)(x)
    x = F.adaptive_avg_pool2d(x, (1, 1))
    return self.fc(torch.flatten(x, 1))  # (dropout in eval mode is the identity)


G.NarrowInception.forward = narrow_forward


def tf_resize(img, size, interpolation=None, antialias=True):
    """TF.resize for a tensor batch and an int size: the shorter side to `size`; BILINEAR where no filter is named."""
    assert isinstance(size, int) and antialias
    mode = RESIZE["default"] if interpolation is None else interpolation.value
    h, w = img.shape[-2:]
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    new_w, new_h = (new_short, new_long) if w <= h else (new_long, new_short)
    if (new_h, new_w) == (h, w):
        return img
    return F.interpolate(img, size=(new_h, new_w), mode=mode, align_corners=False, antialias=True)


def bilinear_prep(x):
    """calculate_inception_score's denormalize + _inception_preprocess in x's dtype; -> NHWC (the GPU test's truth for the kernel)."""
    G.MODE.update(dtype=x.dtype, channels_last=False, resize="antialias")
    v = (x * 0.5 + 0.5).clamp(0, 1)
    v = G.tf_center_crop(tf_resize(v, 299), [299, 299])
    return G.tf_normalize(v, mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225]).permute(0, 2, 3, 1)


class RecordingRng:
    """np.random.default_rng(seed) that keeps what choice() returned."""

    def __init__(self, seed, make):
        self.rng, self.drawn = make(seed), []

    def choice(self, *a, **kw):
        out = self.rng.choice(*a, **kw)
        self.drawn.append(np.array(out))
        return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def peaky_probs(seed, n, c, scale=30.0):
    """float32 softmax rows sharp enough that some entries lie below 1e-16 (the clip acts)."""
    g = torch.Generator().manual_seed(int(seed))
    return torch.softmax(torch.randn((n, c), generator=g, dtype=torch.float64) * scale, dim=1).float().numpy()


def kid_ragged_sets(seed, n_real, n_fake, dim):
    g = torch.Generator().manual_seed(int(seed))
    return (torch.rand((n_real, dim), generator=g) * 1.5).numpy(), (torch.rand((n_fake, dim), generator=g) * 1.5).numpy()


def knn_sets(seed, na, nb, dim):
    """(real [na, dim], fake [nb, dim]) float32: clamped Gaussians, the fake set shifted and narrower."""
    g = torch.Generator().manual_seed(int(seed))
    real = torch.randn((na, dim), generator=g).clamp(-2.0, 2.0)
    fake = (torch.randn((nb, dim), generator=g) * 0.85 + 0.15).clamp(-2.0, 2.0)
    return real.numpy(), fake.numpy()


# ---- the formulas restated, with the switches of the negative checks -----------------------------------------------------------------
def is_formula(probs, splits=10, clip=True, keep_remainder=False):
    p = np.asarray(probs, dtype=np.float64)
    if clip:
        p = np.clip(p, 1e-16, 1.0)
    per = p.shape[0] // splits
    scores = []
    with np.errstate(all="ignore"):
        for i in range(splits):
            part = p[i * per: (i + 1) * per] if not (keep_remainder and i == splits - 1) else p[i * per:]
            if len(part) == 0:
                continue
            py = np.mean(part, axis=0)
            if clip:
                py = np.clip(py, 1e-16, 1.0)
            scores.append(np.exp(np.mean(np.sum(part * (np.log(part) - np.log(py)), axis=1))))
    return np.array([np.mean(scores), np.std(scores)]) if scores else np.array([np.nan, np.nan])


def kid_formula(real, fake, idx_real, idx_fake, gamma, degree, keep_diag=False, divisor_m2=False, clamp=True):
    real, fake = np.asarray(real, np.float64), np.asarray(fake, np.float64)
    vals = []
    for ir, jf in zip(idx_real, idx_fake):
        r, f = real[ir], fake[jf]
        m = len(ir)
        krr, kff, krf = ((gamma * (a @ b.T) + 1.0) ** degree for a, b in ((r, r), (f, f), (r, f)))
        if not keep_diag:
            np.fill_diagonal(krr, 0)
            np.fill_diagonal(kff, 0)
        div = m * m if divisor_m2 else m * (m - 1)
        v = krr.sum() / div + kff.sum() / div - 2.0 * krf.mean()
        vals.append(max(0.0, v) if clamp else v)
    return float(np.mean(vals))


def sq_dists(a, b, dtype):
    a, b = np.asarray(a, dtype), np.asarray(b, dtype)
    if dtype == np.float64:
        return ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    return (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - dtype(2) * (a @ b.T)  # the Gram form, as the kernel takes it


def pr_formula(real, fake, k, dtype=np.float64, exclude_diag=True, kth=None):
    """-> dict of radii, nearest indices and distances (all of the two directions), precision, recall."""
    kth = k if kth is None else kth
    out = {}
    for tag, s in (("real", real), ("fake", fake)):
        d = np.sqrt(np.maximum(sq_dists(s, s, dtype), 0))
        if exclude_diag:
            np.fill_diagonal(d, np.inf)
        out[f"radius_{tag}"] = np.sort(d, axis=1)[:, kth - 1]
    for tag, q, s, rad in (("fake_to_real", fake, real, out["radius_real"]), ("real_to_fake", real, fake, out["radius_fake"])):
        d = np.sqrt(np.maximum(sq_dists(q, s, dtype), 0))
        nn = d.argmin(axis=1)
        srt = np.sort(d, axis=1)
        out[f"nn_{tag}"], out[f"d_{tag}"], out[f"d2_{tag}"] = nn, srt[:, 0], srt[:, 1]
        out[f"hit_{tag}"] = srt[:, 0] <= rad[nn]
        out[f"rad_{tag}"] = rad[nn]
    out["precision"], out["recall"] = float(out["hit_fake_to_real"].mean()), float(out["hit_real_to_fake"].mean())
    return out


def pr_margin(res):
    """The smallest relative margin of a case: nearest distance against the radius it meets, nearest against second nearest."""
    worst = np.inf
    for tag in ("fake_to_real", "real_to_fake"):
        worst = min(worst, (np.abs(res[f"d_{tag}"] - res[f"rad_{tag}"]) / res[f"rad_{tag}"]).min(),
                    ((res[f"d2_{tag}"] - res[f"d_{tag}"]) / res[f"d_{tag}"]).min())
    return float(worst)


def main():
    M = G._reference_metrics()
    sys.modules["torchvision.transforms.functional"].resize = tf_resize
    out = {}

    def mode(dtype=torch.float32, channels_last=False):
        G.MODE.update(dtype=dtype, channels_last=channels_last, resize="antialias")

    # ---- Inception Score --------------------------------------------------------------------------------------------------------
    for i, n in enumerate(IS_CASES):
        seed = SEED + i
        x = G.raw_images(seed, (n, 3, IS_SIDE, IS_SIDE))
        mode()
        ref = np.array(M.calculate_inception_score(x, device="cpu", batch_size=128), dtype=np.float64)
        mode(channels_last=True)
        cl = np.array(M.calculate_inception_score(x, device="cpu", batch_size=128), dtype=np.float64)
        mode(torch.float64)
        f64 = np.array(M.calculate_inception_score(x.double(), device="cpu", batch_size=128), dtype=np.float64)
        with torch.no_grad():  # is_formula (the restatement the negative checks vary) against the reference, on the float64 probabilities
            p64 = torch.softmax(G.narrow_inception().double()(bilinear_prep(x.double()).permute(0, 3, 1, 2)), dim=1).numpy()
        assert np.abs(is_formula(p64) - f64).max() <= 1e-12 * f64[0]
        mode()
        RESIZE["default"] = "bicubic"
        bicubic = np.array(M.calculate_inception_score(x, device="cpu", batch_size=128), dtype=np.float64)
        RESIZE["default"] = "bilinear"
        yard = max(np.abs(ref - f64).max(), np.abs(cl - f64).max())
        print(f"IS n={n}: ref {ref}, f64 {f64}, channels_last {cl}, yardstick {yard:.3e}; bicubic pipeline {bicubic}")
        assert np.abs(bicubic - ref).max() > 40 * yard, "the bicubic pipeline must be told apart"
        out.update({f"is.{n}.seed": np.array(seed), f"is.{n}.ref": ref, f"is.{n}.f64": f64, f"is.{n}.f32_cl": cl,
                    f"is.{n}.yardstick": np.array(yard)})
    probs = peaky_probs(SEED + 10, 37, 13)
    assert (probs < 1e-16).any() and (probs > 0.5).any()
    from_probs = is_formula(probs)
    print(f"IS from stored probabilities [37, 13]: {from_probs}")
    for what, kw in (("no clip", dict(clip=False)), ("remainder kept", dict(keep_remainder=True))):
        wrong = is_formula(probs, **kw)
        print(f"  {what}: {wrong}")
        assert not np.all(np.abs(wrong - from_probs) <= 1e-11 * np.abs(from_probs)), what  # (NaN differs too)
    out.update({"is.probs": probs, "is.from_probs": from_probs})

    # ---- KID ----------------------------------------------------------------------------------------------------------------------
    make_rng = np.random.default_rng
    tiny = np.load(os.path.join(HERE, "inception_tiny.npz"))
    rag = KID_RAGGED
    kid_cases = (("fid48", tiny["fid.features"][0], tiny["fid.features"][1], {}, 50, 50),
                 ("ragged",) + kid_ragged_sets(SEED + 21, rag["n_real"], rag["n_fake"], rag["dim"])
                 + (dict(degree=rag["degree"], gamma=rag["gamma"]), rag["m"], rag["subsets"]))
    for i, (tag, real, fake, kw, m, subsets) in enumerate(kid_cases):
        seed = SEED + 30 + i
        runs = {}
        perm = np.random.RandomState(seed).permutation(real.shape[1])
        for name, (r, f) in (("ref", (real, fake)), ("f64", (real.astype(np.float64), fake.astype(np.float64))),
                             ("f32_perm", (np.ascontiguousarray(real[:, perm]), np.ascontiguousarray(fake[:, perm])))):
            rec = RecordingRng(seed, make_rng)
            np.random.default_rng = lambda *a, rec=rec: rec
            try:
                runs[name] = M.kid_from_features(r, f, subset_size=m, n_subsets=subsets, **kw)
            finally:
                np.random.default_rng = make_rng
            runs[name + ".idx"] = (np.stack(rec.drawn[0::2]), np.stack(rec.drawn[1::2]))
        idx_real, idx_fake = runs["ref.idx"]
        assert idx_real.shape == (subsets, m) and all(np.array_equal(runs[k + ".idx"][0], idx_real) for k in ("f64", "f32_perm"))
        gamma, degree = kw.get("gamma", 1.0 / real.shape[1]), kw.get("degree", 3)
        assert abs(kid_formula(real, fake, idx_real, idx_fake, gamma, degree) - runs["f64"]) <= 1e-12 * abs(runs["f64"])
        yard = max(abs(runs["ref"] - runs["f64"]), abs(runs["f32_perm"] - runs["f64"]))
        print(f"KID {tag}: ref {runs['ref']:.9e}, f64 {runs['f64']:.9e}, permuted {runs['f32_perm']:.9e}, yardstick {yard:.3e}")
        variants = {"diagonals kept": dict(keep_diag=True), "divisor m^2": dict(divisor_m2=True)}
        if tag == "ragged":
            variants["no clamp"] = dict(clamp=False)
        for what, vkw in variants.items():
            wrong = kid_formula(real, fake, idx_real, idx_fake, gamma, degree, **vkw)
            print(f"  {what}: {wrong:.9e}")
            assert abs(wrong - runs["ref"]) > 40 * yard, what
        out.update({f"kid.{tag}.seed": np.array(seed), f"kid.{tag}.idx_real": idx_real.astype(np.int16),
                    f"kid.{tag}.idx_fake": idx_fake.astype(np.int16), f"kid.{tag}.gamma": np.array(gamma), f"kid.{tag}.degree": np.array(degree),
                    f"kid.{tag}.ref": np.array(runs["ref"]), f"kid.{tag}.f64": np.array(runs["f64"]),
                    f"kid.{tag}.f32_perm": np.array(runs["f32_perm"]), f"kid.{tag}.yardstick": np.array(yard)})
    out["kid.ragged.set_seed"] = np.array(SEED + 21)

    # ---- precision / recall ---------------------------------------------------------------------------------------------------
    for tag, (na, nb, dim), k in PR_CASES:
        seed = 11
        while True:
            real, fake = knn_sets(seed, na, nb, dim)
            res = pr_formula(real, fake, k)
            if pr_margin(res) >= MARGIN:
                break
            seed += 1
        ref_p, ref_r = M.precision_recall_from_features(real, fake, k=k)
        ref64 = M.precision_recall_from_features(real.astype(np.float64), fake.astype(np.float64), k=k)
        assert (ref_p, ref_r) == ref64 == (res["precision"], res["recall"]), (ref_p, ref_r, ref64, res["precision"], res["recall"])
        g32 = pr_formula(real, fake, k, dtype=np.float32)
        assert np.array_equal(g32["nn_fake_to_real"], res["nn_fake_to_real"]) and np.array_equal(g32["nn_real_to_fake"], res["nn_real_to_fake"])
        yard = max(np.abs(g32["radius_real"].astype(np.float64) - res["radius_real"]).max(),
                   np.abs(g32["radius_fake"].astype(np.float64) - res["radius_fake"]).max())
        print(f"P/R {tag}: seed {seed}, margin {pr_margin(res):.2e}, precision {ref_p:.6f}, recall {ref_r:.6f}, radius yardstick {yard:.3e}")
        assert 0.0 < ref_p < 1.0 and 0.0 < ref_r < 1.0
        for what, vkw in (("diagonal kept", dict(exclude_diag=False)), ("radius at k + 1", dict(kth=k + 1))):
            wrong = pr_formula(real, fake, k, **vkw)
            print(f"  {what}: precision {wrong['precision']:.6f}, recall {wrong['recall']:.6f}")
            assert (wrong["precision"], wrong["recall"]) != (ref_p, ref_r), what
            assert np.abs(wrong["radius_real"] - res["radius_real"]).max() > 40 * yard, what
        out.update({f"pr.{tag}.seed": np.array(seed), f"pr.{tag}.shape": np.array((na, nb, dim)), f"pr.{tag}.k": np.array(k),
                    f"pr.{tag}.radius_real": res["radius_real"], f"pr.{tag}.radius_fake": res["radius_fake"],
                    f"pr.{tag}.nn_fake_to_real": res["nn_fake_to_real"].astype(np.int32),
                    f"pr.{tag}.nn_real_to_fake": res["nn_real_to_fake"].astype(np.int32),
                    f"pr.{tag}.precision": np.array(ref_p), f"pr.{tag}.recall": np.array(ref_r), f"pr.{tag}.yardstick": np.array(yard)})

    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(f"wrote {OUT} keys={len(out)} bytes={size}")
    assert size < 1_000_000


if __name__ == "__main__":
    main()

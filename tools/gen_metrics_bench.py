#!/usr/bin/env python3
"""Cost of the generative evaluation's feature-space kernels at the reference's sample count, N = 10 000 features of D = 2048 and
C = 1000 classes (seeded random values: the arithmetic does not depend on them), and of the whole stage, each against a plain-torch
composition on the same device in the same process.

Timed, each with device events, a warm-up and the median of --repeats windows, the two sides alternating:
  * the classifier head: ops.linear_softmax            vs  torch.softmax(feat @ W.T + b)
  * the Inception Score: ops.inception_score_splits    vs  clip / mean / log / sum per split in float64 torch ops
  * KID, 50 subsets of 50: ops.kid_subsets             vs  gather + torch.bmm of the three kernel blocks in float64
  * one neighbour search: ops.knn_rows (k = 3, N x N)  vs  torch.cdist + topk
  * precision / recall: metrics.precision_recall_from_features (four searches)  vs  four cdist + topk / min
  * the bilinear input pipeline per 128-image chunk: ops.inception_prep(filter="bilinear")  vs  F.interpolate(antialias=True) + crop
    + normalise
  * the feature-space part of the stage from resident features: gFID (host float64 eigh, the same on both sides and listed on its
    own) + KID + IS + precision / recall
  * the stage end to end, train.evaluate_generative_metrics, on --stage_samples samples of a small VAE at 32 x 32 with random weights
    of the real widths (generation + three Inception passes + the metrics); no torch side: its Inception stack is timed by
    tools/inception_bench.py.
Every pair's outputs are compared and the largest difference is printed with the times.  Prints one JSON line.  bench.py is not
touched.

Usage:  python tools/gen_metrics_bench.py [--n 10000] [--repeats 5] [--stage_samples 10000] [--no-stage]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--stage_samples", type=int, default=10000)
    ap.add_argument("--no-stage", action="store_true")
    a = ap.parse_args()

    import numpy as np
    import torch
    import torch.nn.functional as F

    import movae_amd  # noqa: F401
    from movae_amd import inception, metrics, ops, train

    dev = torch.device("cuda:0")
    n, d, c = a.n, a.dim, a.classes
    g = torch.Generator().manual_seed(0)
    # features like the pooled ReLU outputs of the stack: non-negative, two sets with different statistics
    real = (torch.rand((n, d), generator=g) * torch.rand((1, d), generator=g)).to(dev)
    fake = (torch.rand((n, d), generator=g) * torch.rand((1, d), generator=g) * 0.9 + 0.02).to(dev)
    weight = (torch.randn((c, d), generator=g) * 0.05).to(dev)
    bias = (torch.randn(c, generator=g) * 0.1).to(dev)
    res = {"n": n, "dim": d, "classes": c, "dtype": "fp32"}

    def window(fn, iters):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / iters

    def pair(name, hip, ref, diff, iters=3):
        """Times both sides (ms per call: median, [min, max]) alternating, and records diff(hip(), ref())."""
        outs = [hip(), ref()]  # (the warm-up; also what is compared)
        torch.cuda.synchronize()
        res[f"{name}_max_abs_diff"] = float(diff(*outs))
        del outs
        ts = ([], [])
        for _ in range(a.repeats):
            for t, fn in zip(ts, (hip, ref)):
                t.append(window(fn, iters))
        res[f"{name}_hip_ms"], res[f"{name}_torch_ms"] = statistics.median(ts[0]), statistics.median(ts[1])
        res[f"{name}_hip_spread_ms"], res[f"{name}_torch_spread_ms"] = [min(ts[0]), max(ts[0])], [min(ts[1]), max(ts[1])]
        print(f"{name}: hip {res[f'{name}_hip_ms']:.3f} ms, torch {res[f'{name}_torch_ms']:.3f} ms, max diff {res[f'{name}_max_abs_diff']:.3e}",
              file=sys.stderr, flush=True)

    with torch.no_grad():
        # ---- the head ----
        pair("linear_softmax", lambda: ops.linear_softmax(fake, weight, bias), lambda: torch.softmax(fake @ weight.T + bias, dim=1),
             lambda x, y: (x - y).abs().max())
        probs = ops.linear_softmax(fake, weight, bias)

        # ---- the Inception Score ----
        def torch_is(p, splits=10):
            per = p.size(0) // splits
            q = p[: per * splits].double().clamp(1e-16, 1.0).view(splits, per, -1)
            py = q.mean(1, keepdim=True).clamp(1e-16, 1.0)
            return torch.exp((q * (q.log() - py.log())).sum(2).mean(1))

        pair("inception_score", lambda: ops.inception_score_splits(probs, 10), lambda: torch_is(probs), lambda x, y: (x - y).abs().max())

        # ---- KID ----
        idx_real, idx_fake = metrics.kid_subset_indices(n, n, 50, 50, seed=0)
        ir = torch.from_numpy(idx_real.astype(np.int32)).to(dev)
        jf = torch.from_numpy(idx_fake.astype(np.int32)).to(dev)
        gamma = 1.0 / d

        def torch_kid():
            r, f = real[ir.long()].double(), fake[jf.long()].double()  # [S, m, D]
            m = r.size(1)
            k_rr, k_ff, k_rf = ((gamma * torch.bmm(x, y.transpose(1, 2)) + 1.0) ** 3 for x, y in ((r, r), (f, f), (r, f)))
            off = 1.0 - torch.eye(m, dtype=torch.float64, device=dev)
            v = (k_rr * off).sum((1, 2)) / (m * (m - 1)) + (k_ff * off).sum((1, 2)) / (m * (m - 1)) - 2.0 * k_rf.mean((1, 2))
            return v.clamp_min(0)

        pair("kid_subsets", lambda: ops.kid_subsets(real, fake, ir, jf, gamma, 3), torch_kid, lambda x, y: (x - y).abs().max())

        # ---- nearest neighbours ----
        def torch_knn(x, y, k, exclude):
            dist = torch.cdist(x, y)
            if exclude:
                dist.fill_diagonal_(float("inf"))
            return dist.topk(k, dim=1, largest=False)

        pair("knn_rows_k3", lambda: ops.knn_rows(real, real, 3, exclude_diag=True)[0].sqrt(), lambda: torch_knn(real, real, 3, True)[0],
             lambda x, y: (x - y).abs().max(), iters=1)
        res["knn_rows_k3_tflops"] = 2.0 * n * n * d / (res["knn_rows_k3_hip_ms"] * 1e-3) / 1e12

        def torch_pr(k=3):
            radius_real = torch_knn(real, real, k, True)[0][:, k - 1]
            radius_fake = torch_knn(fake, fake, k, True)[0][:, k - 1]
            d_fr, i_fr = torch.cdist(fake, real).min(dim=1)
            d_rf, i_rf = torch.cdist(real, fake).min(dim=1)
            return torch.stack([(d_fr <= radius_real[i_fr]).float().mean(), (d_rf <= radius_fake[i_rf]).float().mean()])

        pair("precision_recall", lambda: torch.tensor(metrics.precision_recall_from_features(real, fake, k=3)), lambda: torch_pr().cpu(),
             lambda x, y: (x - y).abs().max(), iters=1)

        # ---- the bilinear input pipeline, one chunk ----
        raw = (torch.rand((128, 3, 32, 32), generator=g) * 2 - 1).to(dev)
        mean = torch.tensor([0.485, 0.456, 0.406], device=dev).view(1, 3, 1, 1)
        std = torch.tensor([0.229, 0.224, 0.225], device=dev).view(1, 3, 1, 1)
        buf = torch.empty((128, 299, 299, 3), device=dev)

        def torch_prep():
            v = (raw * 0.5 + 0.5).clamp(0, 1)
            v = F.interpolate(v, size=(299, 299), mode="bilinear", align_corners=False, antialias=True)
            return ((v - mean) / std).permute(0, 2, 3, 1)

        pair("prep_bilinear_chunk128", lambda: ops.inception_prep(raw, buf, filter="bilinear"), torch_prep, lambda x, y: (x - y).abs().max())

        # ---- the feature-space part of the stage, from resident features ----
        def timed_host(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, out

        metrics.fid_from_features(real[:64, :64], fake[:64, :64])  # (warm-up of the eigensolver)
        res["gfid_host_ms"], gfid = timed_host(lambda: metrics.fid_from_features(real, fake))
        res["gfid"] = gfid

        def hip_rest():
            return (metrics.kid_from_features(real, fake, seed=0), metrics.inception_score_from_probs(probs),
                    metrics.precision_recall_from_features(real, fake, k=3))

        def torch_rest():
            return (float(torch_kid().mean().item()), torch_is(probs).cpu().numpy(), torch_pr().cpu().numpy())

        hip_rest(), torch_rest()
        ts = ([], [])
        for _ in range(a.repeats):
            ts[0].append(timed_host(hip_rest)[0])
            ts[1].append(timed_host(torch_rest)[0])
        res["kid_is_pr_hip_ms"], res["kid_is_pr_torch_ms"] = statistics.median(ts[0]), statistics.median(ts[1])
        res["kid_is_pr_hip_spread_ms"], res["kid_is_pr_torch_spread_ms"] = [min(ts[0]), max(ts[0])], [min(ts[1]), max(ts[1])]
    print(json.dumps(res), file=sys.stderr, flush=True)  # (the kernels alone, should the stage not finish)

    # ---- the stage end to end ----
    if not a.no_stage:
        from movae_amd.models import get_network

        sd = inception.random_state_dict(seed=0)
        gg = torch.Generator().manual_seed(1)
        sd["fc.weight"], sd["fc.bias"] = torch.randn((c, 2048), generator=gg) * 0.05, torch.randn(c, generator=gg) * 0.1
        inception.use_inception_weights(sd)
        args = train.parse_args(["--arch", "vae", "--latent_dim", "16", "--hidden_dims", "16", "32", "--batch_size", "128",
                                 "--max_gen_metrics_samples", str(a.stage_samples), "--gen_precision_recall", "--seed", "0"])
        args.dataset_size = 50000
        torch.manual_seed(0)
        net = get_network(32, num_channels=3, args=args, device=dev).to(dev)
        pool = (torch.rand((1024, 3, 32, 32), generator=gg) * 2 - 1).to(dev)
        loader = [(pool[i % 8 * 128: i % 8 * 128 + 128], None) for i in range(-(-a.stage_samples // 128))]
        args.max_gen_metrics_samples = 256
        train.evaluate_generative_metrics(net, loader[:2], dev, args)  # (warm-up of every shape but the last partial chunk)
        args.max_gen_metrics_samples = a.stage_samples
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = train.evaluate_generative_metrics(net, loader, dev, args)
        torch.cuda.synchronize()
        res["stage_samples"], res["stage_s"], res["stage_result"] = a.stage_samples, time.perf_counter() - t0, out
        inception.use_inception_weights(None)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

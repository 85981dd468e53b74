#!/usr/bin/env python3
"""Cost of the Inception-v3 feature extraction behind rFID per 128-sample chunk (128 x 3 x 299 x 299 after the resize), at the real
widths with seeded random weights (inception.random_state_dict: the arithmetic does not depend on the values), fp32.

Timed, each with device events, a warm-up and the median of --repeats windows, the sides alternating:
  * the HIP extractor end to end from 32 x 32 images (metrics.inception_features_into: ops.inception_prep + the stack);
  * its split into stages: prep, stem, Mixed_5b-5d, Mixed_6a-6e, Mixed_7a-7c, global mean;
  * a plain-torch composition of the same stack -- F.conv2d + eval-mode F.batch_norm + relu, F.max_pool2d / F.avg_pool2d, torch.cat
    -- on the same device in the same process, driven by the same topology table, in NCHW and in channels_last memory, with the same
    stage split; its features are compared with the HIP ones.
Also printed: the convolutions' FLOPs per image (2 M N K summed over the 94 layers) and the fraction of the 155 TFLOP/s fp32-MFMA rate
the HIP stack reaches.  Prints one JSON line.  bench.py is not touched.

Usage:  python tools/inception_bench.py [--chunk 128] [--iters 2] [--repeats 5] [--no-torch]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP32_MFMA_TFLOPS = 155.0
STAGES = (("stem", ()), ("Mixed_5", ("Mixed_5b", "Mixed_5c", "Mixed_5d")), ("Mixed_6", ("Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e")),
          ("Mixed_7", ("Mixed_7a", "Mixed_7b", "Mixed_7c")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk", type=int, default=128)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--side", type=int, default=32, help="side of the raw images the end-to-end number starts from")
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()

    import torch
    import torch.nn.functional as F

    import movae_amd  # noqa: F401
    from movae_amd import inception, metrics, ops

    dev = torch.device("cuda:0")
    n = a.chunk
    sd = inception.random_state_dict(seed=0)
    inception.use_inception_weights(sd)
    weights = inception.registered_inception_weights()
    net = metrics._inception_on(dev, weights)
    blocks = dict(inception.BLOCKS)
    res = {"chunk": n, "dtype": "fp32", "feature_dim": net.feature_dim}

    def window(fn, iters):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / iters  # ms per call

    def timed(fns, iters):
        for fn in fns:
            window(fn, 1)
        ts = [[] for _ in fns]
        for _ in range(a.repeats):
            for t, fn in zip(ts, fns):
                t.append(window(fn, iters))
        return [statistics.median(t) for t in ts], [[min(t), max(t)] for t in ts]

    # ---- FLOPs of the convolutions per image at 299 x 299 ----
    def conv_flops():
        total, per_stage = 0, {}
        shape = {"h": 299, "w": 299, "c": 3}

        def conv(h, w, c, name, geom):
            kh, kw, s, ph, pw = geom
            co = weights[f"{name}.weight"].shape[0]
            ho, wo = ops.conv_out_size(h, kh, s, ph), ops.conv_out_size(w, kw, s, pw)
            return ho, wo, co, 2 * ho * wo * co * kh * kw * c

        h, w, c = shape["h"], shape["w"], shape["c"]
        fl = 0
        for step in inception.STEM:
            if step == "max":
                h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
            else:
                h, w, c, f = conv(h, w, c, step[0], step[1])
                fl += f
        per_stage["stem"] = fl
        total += fl
        for stage, names in STAGES[1:]:
            fl = 0
            for block in names:
                seen, widths, oh, ow = set(), 0, h, w
                for path in blocks[block]:
                    ph_, pw_, pc = h, w, c
                    for i, step in enumerate(path):
                        if step == "max":
                            ph_, pw_ = (ph_ - 3) // 2 + 1, (pw_ - 3) // 2 + 1
                        elif step != "avg":
                            ph_, pw_, pc, f = conv(ph_, pw_, pc, f"{block}.{step[0]}", step[1])
                            if path[: i + 1] not in seen:
                                seen.add(path[: i + 1])
                                fl += f
                    widths += pc
                    oh, ow = ph_, pw_
                h, w, c = oh, ow, widths
            per_stage[stage] = fl
            total += fl
        return total, per_stage

    flops, stage_flops = conv_flops()
    res["conv_gflop_per_image"] = flops / 1e9
    res["stage_gflop_per_image"] = {k: v / 1e9 for k, v in stage_flops.items()}
    res["floor_ms_per_chunk_at_155TF"] = flops * n / (FP32_MFMA_TFLOPS * 1e12) * 1e3

    # ---- the HIP extractor ----
    g = torch.Generator().manual_seed(1)
    raw = (torch.rand(n, 3, a.side, a.side, generator=g) * 2 - 1).to(dev)
    out = torch.empty(n, net.feature_dim, dtype=torch.float32, device=dev)
    shape = (n, ops.INCEPTION_SIDE, ops.INCEPTION_SIDE, 3)
    net._select(shape)
    x299 = ops.inception_prep(raw).clone()

    def hip_stage(stage, names, x):
        if stage == "stem":
            for i, step in enumerate(inception.STEM):
                x = net._pool(x, "max", f"stem.max{i}", None, 0) if step == "max" else net._conv(x, step[0], step[1], None, 0)
            return x
        for block in names:
            x = net._block(x, block, blocks[block])
        return x

    net._select(shape)
    hip_in, x = {}, x299
    for stage, names in STAGES:
        hip_in[stage] = x
        x = hip_stage(stage, names, x)
    hip_last = x
    hip_feat = ops.infer_global_mean(hip_last).clone()

    fns = [lambda: metrics.inception_features_into(out, raw, n), lambda: net(x299), lambda: ops.inception_prep(raw, net._buf("prep", shape))]
    fns += [(lambda s=stage, nm=names: hip_stage(s, nm, hip_in[s])) for stage, names in STAGES]
    fns += [lambda: ops.infer_global_mean(hip_last)]
    med, spread = timed(fns, a.iters)
    keys = ["end_to_end", "stack", "prep"] + [s for s, _ in STAGES] + ["global_mean"]
    res["hip_ms"] = dict(zip(keys, med))
    res["hip_spread_ms"] = dict(zip(keys, spread))
    res["hip_images_per_s"] = n / (med[0] * 1e-3)
    res["hip_stack_tflops"] = flops * n / (med[1] * 1e-3) / 1e12
    res["hip_stack_fraction_of_155TF"] = res["hip_stack_tflops"] / FP32_MFMA_TFLOPS
    res["hip_stage_tflops"] = {s: stage_flops[s] * n / (res["hip_ms"][s] * 1e-3) / 1e12 for s, _ in STAGES}

    print(json.dumps(res), file=sys.stderr, flush=True)  # (the HIP side alone, should the torch side not finish)

    # ---- the plain-torch composition of the same table ----
    if not a.no_torch:
        tsd = {k: v.to(dev) for k, v in sd.items()}

        def tconv(x, name, geom):
            kh, kw, s, ph, pw = geom
            y = F.conv2d(x, tsd[f"{name}.conv.weight"], stride=s, padding=(ph, pw))
            y = F.batch_norm(y, tsd[f"{name}.bn.running_mean"], tsd[f"{name}.bn.running_var"], tsd[f"{name}.bn.weight"], tsd[f"{name}.bn.bias"],
                             False, 0.0, inception.BN_EPS)
            return F.relu(y)

        def tpool(x, mode):
            return F.max_pool2d(x, 3, stride=2) if mode == "max" else F.avg_pool2d(x, 3, stride=1, padding=1)

        def torch_stage(stage, names, x):
            if stage == "stem":
                for step in inception.STEM:
                    x = tpool(x, "max") if step == "max" else tconv(x, step[0], step[1])
                return x
            for block in names:
                done, outs = {}, []
                for path in blocks[block]:
                    cur = x
                    for i, step in enumerate(path):
                        key = path[: i + 1]
                        if key not in done:
                            done[key] = tpool(cur, step) if step in ("max", "avg") else tconv(cur, f"{block}.{step[0]}", step[1])
                        cur = done[key]
                    outs.append(cur)
                x = torch.cat(outs, 1)
            return x

        def torch_stack(x):
            for stage, names in STAGES:
                x = torch_stage(stage, names, x)
            return x.mean((2, 3))

        for fmt_name, fmt in (("nchw", torch.contiguous_format), ("channels_last", torch.channels_last)):
            with torch.no_grad():
                tx = x299.permute(0, 3, 1, 2).contiguous(memory_format=fmt)
                for k in tsd:
                    if k.endswith("conv.weight"):
                        tsd[k] = tsd[k].contiguous(memory_format=fmt)
                t_in, x = {}, tx
                for stage, names in STAGES:
                    t_in[stage] = x
                    x = torch_stage(stage, names, x)
                t_feat = x.mean((2, 3))
                res[f"torch_{fmt_name}_max_abs_diff_vs_hip"] = float((t_feat - hip_feat).abs().max().item())
                res[f"torch_{fmt_name}_feature_max_abs"] = float(t_feat.abs().max().item())
                fns = [lambda: torch_stack(tx)] + [(lambda s=stage, nm=names: torch_stage(s, nm, t_in[s])) for stage, names in STAGES]
                med, spread = timed(fns, a.iters)
            keys = ["stack"] + [s for s, _ in STAGES]
            res[f"torch_{fmt_name}_ms"] = dict(zip(keys, med))
            res[f"torch_{fmt_name}_spread_ms"] = dict(zip(keys, spread))
            res[f"torch_{fmt_name}_stack_tflops"] = flops * n / (med[0] * 1e-3) / 1e12
    inception.use_inception_weights(None)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Training the PixelCNN priors on one MI355X: steps per second of the prior stage's loop (prior.train_pixelcnn_prior) on three paths,
in the same process and alternating:

  host_eager    today's path: torch DataLoader (num_workers=0) over the host VQCodeDataset, .to(device), the eager step
  device_eager  prior.DeviceCodeLoader (one movae_codes_batch launch per batch), the eager step
  device_graph  DeviceCodeLoader bound to the static inputs of prior.GraphedPriorStep: one launch and one hipGraph replay per step

Shapes (main.py's prior defaults: K 512, D 64, hidden 128, 15 layers):
  flat  the flat prior on 16x16 codes at B = 128
  hier  the hierarchical prior on 32x32 + 64x64 codes at B = 8 (the batch size of bench.py's C4)

Host clock around --steps steps that end in a device synchronise, after a warm-up of each path; the per-step losses stay on the device
like the stage's.  --reps repetitions per path, the median and every run reported.  `launches` counts C-ABI launches of one step
(_lib.TRACE; for the graph path: the launches inside the captured graph, and what the host still issues per step).  Before timing,
the graph path is compared with the eager step on the same batches (`worst_loss_diff`, `worst_param_diff` after --check-steps steps).
One JSON line.  Needs the GPU: there is no fallback.

Usage:  python tools/prior_train_bench.py [--reps 3] [--steps 200] [--only flat|hier]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, D, HIDDEN, LAYERS = 512, 64, 128, 15
SHAPES = {"flat": dict(hier=False, grids=((16, 16),), B=128, n=4096), "hier": dict(hier=True, grids=((32, 32), (64, 64)), B=8, n=512)}
PATHS = ("host_eager", "device_eager", "device_graph")


def make_prior(hier, dev, device_step):
    import torch

    from movae_amd.models.pixelcnn_prior import HierarchicalPixelCNN, PixelCNN
    from movae_amd.optim import FusedAdam

    torch.manual_seed(0)
    net = (HierarchicalPixelCNN if hier else PixelCNN)(K, D, HIDDEN, LAYERS).to(dev).train()
    return net, FusedAdam(net.parameters(), lr=3e-4, weight_decay=0.0, device_step=device_step)


class Path:
    """One of the three loops, with a prior and an optimizer of its own: run(steps) makes that many steps, epoch after epoch."""

    def __init__(self, name, ds, cfg, dev):
        import torch

        from movae_amd import prior as P

        self.name, self.hier, self.dev, self.epoch, self.graphed = name, cfg["hier"], dev, 0, None
        self.net, self.opt = make_prior(cfg["hier"], dev, device_step=name == "device_graph")
        if name == "host_eager":
            self.loader = torch.utils.data.DataLoader(ds, batch_size=cfg["B"], shuffle=True, num_workers=0, drop_last=False)
        else:
            self.loader = P.DeviceCodeLoader(ds, cfg["B"], dev, shuffle=True, seed=0)
        if name == "device_graph":
            first = next(iter(self.loader))
            first = first if self.hier else (first,)
            self.graphed = P.GraphedPriorStep(self.net, self.opt, *first, record_calls=True)
            self.loader.bind(self.graphed.static_top, self.graphed.static_bottom)

    def batches(self):
        while True:
            self.epoch += 1
            if hasattr(self.loader, "set_epoch"):
                self.loader.set_epoch(self.epoch)
            for b in self.loader:
                b = tuple(b) if self.hier else ((b if hasattr(b, "shape") else b[0]),)
                yield tuple(t.to(self.dev) for t in b) if self.name == "host_eager" else b

    def run(self, steps):
        from movae_amd.prior import _one_step

        losses = []
        for _, b in zip(range(steps), self.batches()):
            losses.append(self.graphed.step(*b) if self.graphed is not None else _one_step(self.net, self.opt, *b))
        return losses


def wall_ms(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def count_launches(path):
    """C-ABI launches of one step of `path` (loader included)."""
    from movae_amd import _lib as L

    calls = []
    L.TRACE = lambda name, cargs: calls.append(name)
    try:
        path.run(1)
    finally:
        L.TRACE = None
    return calls


def check_graph_against_eager(cfg, ds, dev, steps):
    """GraphedPriorStep against the eager step (both FusedAdam(device_step=True)) on the same batches, from the same initial state."""
    import torch

    from movae_amd import prior as P

    loader = P.DeviceCodeLoader(ds, cfg["B"], dev, shuffle=True, seed=1)
    batches = []
    for b in loader:
        batches.append(tuple(b) if cfg["hier"] else (b,))
        if len(batches) == steps:
            break
    net_e, opt_e = make_prior(cfg["hier"], dev, True)
    net_g, opt_g = make_prior(cfg["hier"], dev, True)
    gs = P.GraphedPriorStep(net_g, opt_g, *batches[0])
    dl = 0.0
    for b in batches:
        le, lg = P._one_step(net_e, opt_e, *b), gs.step(*b)
        dl = max(dl, abs(le.item() - lg.item()))
    dp = max((p - q).abs().max().item() for p, q in zip(net_e.parameters(), net_g.parameters()))
    assert gs.replayed_steps == len(batches)
    del gs
    torch.cuda.synchronize()
    return {"steps": len(batches), "worst_loss_diff": dl, "worst_param_diff": dp}


def shape(tag, a, dev):
    import torch

    from movae_amd.prior import VQCodeDataset

    cfg = SHAPES[tag]
    g = torch.Generator().manual_seed(5)
    codes = tuple(torch.randint(0, K, (cfg["n"],) + s, generator=g).to(torch.int16) for s in cfg["grids"])
    ds = VQCodeDataset(codes, cfg["hier"])
    rec = {"B": cfg["B"], "codes": "+".join(f"{h}x{w}" for h, w in cfg["grids"]), "stored_grids": cfg["n"],
           "graph_vs_eager": check_graph_against_eager(cfg, ds, dev, a.check_steps)}
    paths = {name: Path(name, ds, cfg, dev) for name in PATHS}
    for p in paths.values():  # warm-up: every path, before any timing
        p.run(a.warmup)
    torch.cuda.synchronize()
    runs = {name: [] for name in PATHS}
    for _ in range(a.reps):
        for name in PATHS:  # alternating: a drift of the machine lands on every path alike
            runs[name].append(wall_ms(lambda: paths[name].run(a.steps)) / a.steps)
    for name in PATHS:
        ms = statistics.median(runs[name])
        calls = count_launches(paths[name])
        rec[name] = {"ms_per_step": round(ms, 4), "steps_per_s": round(1e3 / ms, 1), "ms_per_step_runs": [round(r, 4) for r in runs[name]],
                     "launches": len(calls)}
    gs = paths["device_graph"].graphed
    rec["device_graph"]["launches_in_graph"] = len(gs.calls)
    rec["device_graph"]["host_issues_per_step"] = "1 movae_codes_batch + 1 graph replay + 1 clone of the loss scalar"
    assert gs.eager_steps == 0, "a timed batch took the eager branch"
    base = rec["host_eager"]["ms_per_step_runs"]
    for name in PATHS[1:]:
        ratios = [b / r for b, r in zip(base, rec[name]["ms_per_step_runs"])]  # per repetition, neighbours in time
        rec[name]["speedup_vs_host_eager"] = round(rec["host_eager"]["ms_per_step"] / rec[name]["ms_per_step"], 3)
        rec[name]["speedup_runs"] = [round(r, 3) for r in ratios]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200, help="timed steps per path per repetition (at least 200 for a number to quote)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--check-steps", type=int, default=8)
    ap.add_argument("--only", choices=sorted(SHAPES), default=None)
    a = ap.parse_args()

    import torch

    import movae_amd  # noqa: F401

    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    out = {"tool": "prior_train_bench", "reps": a.reps, "steps": a.steps, "warmup": a.warmup,
           "prior": {"K": K, "D": D, "hidden": HIDDEN, "layers": LAYERS}}
    for tag in sorted(SHAPES):
        if a.only in (None, tag):
            out[tag] = shape(tag, a, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

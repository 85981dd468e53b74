#!/usr/bin/env python3
"""Golden vectors of the PixelSNAIL priors (runs ONLY in the build container, never on the GPU box).

Imports the reference's models/pixelcnn_prior.py by path (it needs torch only) and records, on the CPU, in the style of
generate_golden.pixelcnn_fixture:
  flat  PixelSNAIL(K=16, D=8, hidden 16, 2 blocks, 1 residual block, 2 heads -> head_dim 8, dropout 0) on a 6x7 grid (L = 42), B=3
  hier  HierarchicalPixelSNAIL(same sizes, 2 bottom PixelCNN layers, dropout 0) on 4x4 top / 8x8 bottom codes, B=2
  eval  the flat sizes with the default dropout 0.1: init state_dict and eval-mode logits
For flat and hier: the init state_dict, logits, losses, every gradient, clip_grad_norm_(1.0), one Adam(3e-4) step, and the second
loss and state_dict (main.py:995-1011).

Usage:  python tests/golden/generate_pixelsnail.py        (seconds)
"""
import importlib.util
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("MOVAE_REFERENCE", "/root/reference")

K, D, HID, BLOCKS, RES, HEADS, LAYERS_BOTTOM, SEED, LR = 16, 8, 16, 2, 1, 2, 2, 11, 3e-4


def _np(t):
    return t.detach().cpu().numpy().copy()


def _ref_module():
    spec = importlib.util.spec_from_file_location("_ref_pixelcnn_prior", os.path.join(REF, "models", "pixelcnn_prior.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    R = _ref_module()
    torch.set_num_threads(8)
    out = {}
    g = torch.Generator().manual_seed(110)
    z = torch.randint(0, K, (3, 6, 7), generator=g)
    z_top = torch.randint(0, K, (2, 4, 4), generator=g)
    z_bot = torch.randint(0, K, (2, 8, 8), generator=g)
    out["meta"] = np.array([f"num_embeddings={K}", f"embedding_dim={D}", f"hidden_channels={HID}", f"num_blocks={BLOCKS}",
                            f"num_res_blocks_per_layer={RES}", f"num_heads={HEADS}", f"num_layers_bottom={LAYERS_BOTTOM}",
                            f"seed={SEED}", f"lr={LR}"])
    out["z"], out["z_top"], out["z_bottom"] = _np(z), _np(z_top), _np(z_bot)
    for tag, hier in (("flat", False), ("hier", True)):
        torch.manual_seed(SEED)
        if hier:
            net = R.HierarchicalPixelSNAIL(K, D, HID, num_blocks_top=BLOCKS, num_res_blocks_per_layer=RES, num_heads=HEADS,
                                           num_layers_bottom=LAYERS_BOTTOM, dropout=0.0)
        else:
            net = R.PixelSNAIL(K, D, HID, num_blocks=BLOCKS, num_res_blocks_per_layer=RES, num_heads=HEADS, dropout=0.0)
        net.train()
        for k, v in net.state_dict().items():
            out[f"{tag}.sd0.{k}"] = _np(v)
        opt = torch.optim.Adam(net.parameters(), lr=LR, weight_decay=0.0)
        opt.zero_grad()
        if hier:
            o = net(z_top, z_bot)
            ld = net.loss_function(z_top, z_bot)
            out[f"{tag}.logits_top"], out[f"{tag}.logits_bottom"] = _np(o["logits_top"]), _np(o["logits_bottom"])
        else:
            logits = net(z)
            ld = {"total_loss": F.cross_entropy(logits.permute(0, 2, 3, 1).reshape(-1, K), z.reshape(-1))}
            out[f"{tag}.logits"] = _np(logits)
        for k, v in ld.items():
            out[f"{tag}.loss.{k}"] = _np(v)
        ld["total_loss"].backward()
        for n, p in net.named_parameters():
            out[f"{tag}.g.{n}"] = _np(p.grad if p.grad is not None else torch.zeros_like(p))
        out[f"{tag}.gnorm"] = _np(torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0))
        opt.step()
        if hier:
            ld2 = net.loss_function(z_top, z_bot)
        else:
            ld2 = {"total_loss": F.cross_entropy(net(z).permute(0, 2, 3, 1).reshape(-1, K), z.reshape(-1))}
        for k, v in ld2.items():
            out[f"{tag}.loss2.{k}"] = _np(v)
        for k, v in net.state_dict().items():
            out[f"{tag}.sd1.{k}"] = _np(v)
        print("pixelsnail", tag, {k: float(v.detach()) for k, v in ld.items()}, {k: float(v.detach()) for k, v in ld2.items()})
    torch.manual_seed(SEED + 1)
    net = R.PixelSNAIL(K, D, HID, num_blocks=BLOCKS, num_res_blocks_per_layer=RES, num_heads=HEADS).eval()  # default dropout 0.1
    for k, v in net.state_dict().items():
        out[f"eval.sd0.{k}"] = _np(v)
    with torch.no_grad():
        out["eval.logits"] = _np(net(z))
    path = os.path.join(HERE, "pixelsnail_tiny.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

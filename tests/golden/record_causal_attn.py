#!/usr/bin/env python3
"""Recorder of tests/golden/causal_attn_parent.npz: the outputs of movae_causal_attn_fwd / _bwd of a GIVEN build of libmovae_hip.so on
two fixed inputs (B 2, heads 3, L 40, hd 6, no dropout; B 1, heads 2, L 33, hd 24, p 0.25 with seed 1234, draw 7), on an MI355X.  The
committed file was recorded from the library built at commit 261b44f ("Add the conv Sphere Encoder ..."), the last one before the
attention kernels were generalised; test_sphere_encoder_vit.py holds the current build to it bit for bit.  The library is loaded by
path through ctypes, not through the package, so a build of another commit can be given.

Usage:  python tests/golden/record_causal_attn.py <path to libmovae_hip.so of the commit to record> tests/golden/causal_attn_parent.npz
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

lib = C.CDLL(os.path.abspath(sys.argv[1]))
out_path = sys.argv[2]
_p, _i, _f, _l, _z, _u = C.c_void_p, C.c_int, C.c_float, C.c_long, C.c_size_t, C.c_ulonglong
lib.movae_causal_attn_fwd.argtypes = [_p, _p, _p, _l, _p, _p, _i, _i, _i, _i, _f, _u, _u, _p]
lib.movae_causal_attn_bwd.argtypes = [_p, _p, _p, _l, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _f, _u, _u, _p, _z, _p]
lib.movae_causal_attn_ws_bytes.argtypes = [_i, _i, _i]
lib.movae_causal_attn_ws_bytes.restype = _z
dev = torch.device("cuda:0")
st = torch.cuda.current_stream(dev).cuda_stream
rec = {}
for tag, (B, heads, L, hd, p, seed, draw) in {"a": (2, 3, 40, 6, 0.0, 0, 0), "b": (1, 2, 33, 24, 0.25, 1234, 7)}.items():
    g = torch.Generator().manual_seed(4242 + L)
    proj = heads * hd
    q, k, v, do = (torch.randn(B, L, proj, generator=g) for _ in range(4))
    qd, kd, vd, dod = (t.to(dev) for t in (q, k, v, do))
    o = torch.empty_like(qd)
    lse = torch.empty(B * heads, L, device=dev)
    assert lib.movae_causal_attn_fwd(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), proj, o.data_ptr(), lse.data_ptr(), B, heads, L, hd, p, seed, draw, st) == 0
    ws = torch.zeros(lib.movae_causal_attn_ws_bytes(B, heads, L), dtype=torch.uint8, device=dev)
    dq, dk, dv = (torch.empty_like(qd) for _ in range(3))
    assert lib.movae_causal_attn_bwd(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), proj, o.data_ptr(), dod.data_ptr(), lse.data_ptr(), dq.data_ptr(),
                                     dk.data_ptr(), dv.data_ptr(), B, heads, L, hd, p, seed, draw, ws.data_ptr(), ws.numel(), st) == 0
    torch.cuda.synchronize()
    rec[tag + ".cfg"] = np.array([B, heads, L, hd, seed, draw], dtype=np.int64)
    rec[tag + ".p"] = np.array(p, dtype=np.float32)
    for n, t in (("q", q), ("k", k), ("v", v), ("dout", do), ("out", o), ("lse", lse), ("dq", dq), ("dk", dk), ("dv", dv)):
        rec[f"{tag}.{n}"] = t.cpu().numpy()
    assert all(np.isfinite(rec[f"{tag}.{n}"]).all() for n in ("out", "lse", "dq", "dk", "dv"))
os.makedirs(os.path.dirname(out_path), exist_ok=True)
np.savez_compressed(out_path, **rec)
print("recorded", out_path, os.path.getsize(out_path))

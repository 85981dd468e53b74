#!/usr/bin/env python3
"""Recorder of tests/golden/conv_pair_parent.json: what movae_conv[T]2d_dgrad_wgrad_grouped_f of a GIVEN build of libmovae_hip.so
dispatches to and computes, on an MI355X.  The committed file was recorded from the library built at commit 2b9f60c ("Exact tests
for the big conv tiles ..."), the last one before the host code that plans and pairs these launches was consolidated;
test_conv_pair_parent.py replays the same cases on the current build and holds it to every recorded field.  The kernels fold in a
fixed order and use no float atomics, so the results are recorded as SHA-256 of their bytes.  The library is loaded by path through
ctypes, not through the package, so a build of another commit can be given -- but run the recorder with the _lib.MovaeFuse of the
SAME commit as the library it records: movae_fuse_t has since lost its last members, and an older library writes an output field of
its own past the end of the shorter struct.

Cases (ids "<row of PAIR_SHAPES>-g<groups>-k<force_kgemm>-<variant>"): every row of test_hip_ops.PAIR_SHAPES, 1 and 2 cotangent
groups, movae_bench_force_kgemm 0 and 1, with no fuse struct ("plain"), with an ep_act ReLU request ("act") and ep_res on top of it
("actres"), and, where ci % 4 == 0, with a bn_* request ("bn"); and the layer chains of
test_hip_deferred_reduce.test_parked_reduce_rides_on_the_next_launch_bit_exact with every weight-gradient reduce armed ("chain<i>").

Usage:  python tests/golden/record_conv_pair.py <path to libmovae_hip.so of the commit to record> tests/golden/conv_pair_parent.json
"""
import ctypes as C
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
RELU = 2
WS_BYTES = 96 << 20
BN_PART_SLOTS = 256  # partial pairs per group and column the bn_* request has room for
CHAINS = [  # (sizes, n, hw, G, force_kgemm): the parametrisation of test_parked_reduce_rides_on_the_next_launch_bit_exact
    ([(64, 128), (128, 64), (64, 128)], 8, 8, 2, 0),
    ([(128, 256), (256, 128), (128, 256)], 16, 4, 2, 1),
    ([(32, 128), (128, 32), (32, 128)], 4, 16, 1, 0),
    ([(256, 256), (256, 256)], 2, 32, 1, 0),
]
ENTRY_POINTS = ["movae_conv2d_dgrad_wgrad_grouped_f", "movae_convT2d_dgrad_wgrad_grouped_f", "movae_conv2d_dgrad_wgrad_grouped",
                "movae_bench_force_kgemm", "movae_bench_last_kernel", "movae_reduce_defer", "movae_reduce_flush", "movae_reduce_defer_stats",
                "movae_reduce_defer_max_bytes", "movae_last_error"]


def pair_shapes():
    sys.path.insert(0, os.path.dirname(HERE))
    try:
        from test_hip_ops import PAIR_SHAPES
    finally:
        sys.path.pop(0)
    return PAIR_SHAPES


def bind(lib, signatures):
    for name in ENTRY_POINTS:
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = signatures[name]
    return lib


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def defer_stats(lib, reset=False):
    out = (C.c_longlong * 3)()
    pending = lib.movae_reduce_defer_stats(out, 1 if reset else 0)
    return list(out), pending


class Arenas:
    """scratch as _lib.workspace hands it out: zero-filled once, arena 0 for ordinary calls, two more in turn for armed ones"""

    def __init__(self, dev):
        self.ws = [torch.zeros(WS_BYTES, dtype=torch.uint8, device=dev) for _ in range(3)]
        self.turn = 0

    def plain(self):
        return self.ws[0].data_ptr(), WS_BYTES

    def armed(self, lib):
        self.turn ^= 1
        lib.movae_reduce_defer(1)
        return self.ws[1 + self.turn].data_ptr(), WS_BYTES


def shape_case_ids(shapes):
    for i, shape in enumerate(shapes):
        for groups in (1, 2):
            for kg in (0, 1):
                for variant in ("plain", "act", "actres") + (("bn",) if shape[4] % 4 == 0 else ()):
                    yield f"{i}-g{groups}-k{kg}-{variant}", (shape, groups, kg, variant)


def run_shape_case(lib, Fuse, arenas, dev, shape, groups, kg, variant):
    tr, n, hi, wi, ci, ho, wo, co, k, stride, pad = shape
    g = torch.Generator().manual_seed(7)
    dy = torch.randn(groups, n, ho, wo, co, generator=g).to(dev)
    x = torch.randn(n, hi, wi, ci, generator=g).to(dev)
    w = ((torch.randn(ci, k, k, co, generator=g) if tr else torch.randn(co, k, k, ci, generator=g)) * 0.1).to(dev)
    side = torch.randn(n, hi, wi, ci, generator=g).to(dev)           # ep_act_y / bn_y: shared by the groups
    res = torch.randn(groups, n, hi, wi, ci, generator=g).to(dev)    # ep_res: one per element of dx
    scale, shift = (torch.rand(ci, generator=g) + 0.5).to(dev), (torch.randn(ci, generator=g) * 0.2).to(dev)
    dx = torch.full((groups, n, hi, wi, ci), float("nan"), device=dev)
    dws = [torch.full_like(w, float("nan")) for _ in range(groups)]
    dbs = [torch.full((co,), float("nan"), device=dev) for _ in range(groups)]
    part = torch.full((groups * BN_PART_SLOTS * 2 * ci,), float("nan"), device=dev)
    f = Fuse()
    if variant in ("act", "actres"):
        f.ep_act_y, f.ep_act, f.ep_slope = side.data_ptr(), RELU, 0.0
        if variant == "actres":
            f.ep_res = res.data_ptr()
    elif variant == "bn":
        f.bn_y, f.bn_scale, f.bn_shift, f.bn_slope = side.data_ptr(), scale.data_ptr(), shift.data_ptr(), 0.01
        f.bn_part, f.bn_cap = part.data_ptr(), part.numel()
    arr = C.c_void_p * groups
    wsp, wsb = arenas.plain()
    st = torch.cuda.current_stream(dev).cuda_stream
    prev = lib.movae_bench_force_kgemm(kg)
    try:
        defer_stats(lib, reset=True)
        rc = getattr(lib, ("movae_convT2d_" if tr else "movae_conv2d_") + "dgrad_wgrad_grouped_f")(
            groups, dy.data_ptr(), w.data_ptr(), x.data_ptr(), dx.data_ptr(), arr(*[t.data_ptr() for t in dws]),
            arr(*[t.data_ptr() for t in dbs]), n, hi, wi, ci, ho, wo, co, k, k, stride, pad, 0, wsp, wsb, st,
            None if variant == "plain" else C.byref(f))
        assert rc == 0, lib.movae_last_error().decode(errors="replace")
        kernel = lib.movae_bench_last_kernel().decode()
        stats, pending = defer_stats(lib)
    finally:
        lib.movae_bench_force_kgemm(prev)
    torch.cuda.synchronize()
    return {"kernel": kernel, "bn_ppg": f.bn_ppg, "ep_act_done": f.ep_act_done, "stats_parts": f.stats_parts,
            "defer_stats": stats + [pending], "dx": sha(dx), "dw": [sha(t) for t in dws], "db": [sha(t) for t in dbs],
            "bn_part": sha(part[:groups * f.bn_ppg * 2 * ci])}


def run_chain_case(lib, arenas, dev, sizes, n, hw, G, kg):
    def rnd(*shape, seed):
        return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))

    st = torch.cuda.current_stream(dev).cuda_stream
    prev = lib.movae_bench_force_kgemm(kg)
    prev_max = lib.movae_reduce_defer_max_bytes(1 << 40)  # park whatever the layer produces
    layers = []
    try:
        defer_stats(lib, reset=True)
        for i, (ci, co) in enumerate(sizes):
            x = rnd(n, hw, hw, ci, seed=10 + i).to(dev)
            w = (rnd(co, ci, 3, 3, seed=20 + i) * 0.1).to(dev).permute(0, 2, 3, 1).contiguous()
            dy = rnd(G, n, hw, hw, co, seed=30 + i).to(dev)
            dx = torch.full((G, n, hw, hw, ci), float("nan"), device=dev)
            dws = [torch.full((co, 3, 3, ci), float("nan"), device=dev) for _ in range(G)]
            wsp, wsb = arenas.armed(lib)
            rc = lib.movae_conv2d_dgrad_wgrad_grouped(G, dy.data_ptr(), w.data_ptr(), x.data_ptr(), dx.data_ptr(),
                                                      (C.c_void_p * G)(*[t.data_ptr() for t in dws]), None, n, hw, hw, ci, hw, hw, co, 3, 3,
                                                      1, 1, 0, wsp, wsb, st)
            assert rc == 0, lib.movae_last_error().decode(errors="replace")
            layers.append((lib.movae_bench_last_kernel().decode(), dx, dws))
        stats, pending = defer_stats(lib)
        assert lib.movae_reduce_flush() == 0
    finally:
        lib.movae_reduce_defer_max_bytes(prev_max)
        lib.movae_bench_force_kgemm(prev)
    torch.cuda.synchronize()
    return {"kernel": [k for k, _, _ in layers], "defer_stats": stats + [pending], "dx": [sha(dx) for _, dx, _ in layers],
            "dw": [[sha(t) for t in dws] for _, _, dws in layers]}


def cases(shapes):
    """id -> function(lib, Fuse, arenas, dev) -> record"""
    out = {}
    for cid, (shape, groups, kg, variant) in shape_case_ids(shapes):
        out[cid] = lambda lib, Fuse, arenas, dev, a=(shape, groups, kg, variant): run_shape_case(lib, Fuse, arenas, dev, *a)
    for i, chain in enumerate(CHAINS):
        out[f"chain{i}"] = lambda lib, Fuse, arenas, dev, a=chain: run_chain_case(lib, arenas, dev, *a)
    return out


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import movae_amd  # noqa: F401  (the binding's types only: nothing is loaded through the package)
    from movae_amd import _lib

    lib = bind(C.CDLL(os.path.abspath(sys.argv[1])), _lib.SIGNATURES)
    dev = torch.device("cuda:0")
    arenas = Arenas(dev)
    rec = {cid: fn(lib, _lib.MovaeFuse, arenas, dev) for cid, fn in cases(pair_shapes()).items()}
    with open(sys.argv[2], "w") as fh:
        json.dump({"cases": rec}, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print("recorded", sys.argv[2], len(rec), "cases", os.path.getsize(sys.argv[2]), "bytes")


if __name__ == "__main__":
    main()

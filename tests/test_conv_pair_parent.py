"""The dgrad + wgrad entry points against a recording of the build before their host code (the stash of the planned input gradient,
the side-product plan, the entry-point bodies) was consolidated: tests/golden/conv_pair_parent.json, written by
tests/golden/record_conv_pair.py from that build on an MI355X.  Only host code changed, the kernels fold in a fixed order and use no
float atomics, so every recorded field -- the kernel the call dispatched to, what the fuse struct reports back, the deferred-reduce
counters and the SHA-256 of every result -- must come out the same.  The twelve records of the first conv (3 -> 32, 3x3, stride 2)
had their kernel field respelled from the two per-dispatch-site labels of the thin-channel family to the launched instantiations,
"thin_out_tile_k<true,32,1> + thin_wgrad_mfma_k<3,3,3,false>", when movae_bench_last_kernel() began to name those (one label used
to cover several kernels there); nothing else in the recording changed.  GPU only."""
import importlib.util
import json
import os

import pytest

from test_hip_ops import PAIR_SHAPES

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
_spec = importlib.util.spec_from_file_location("record_conv_pair", os.path.join(GOLDEN, "record_conv_pair.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)
CASES = rec.cases(PAIR_SHAPES)
with open(os.path.join(GOLDEN, "conv_pair_parent.json")) as _fh:
    RECORDED = json.load(_fh)["cases"]


@pytest.fixture(scope="module")
def bound(gpu_device):
    import movae_amd  # noqa: F401
    from movae_amd import _lib as L

    return L.load(), L.MovaeFuse, rec.Arenas(gpu_device)


def test_the_recording_covers_every_case():
    assert sorted(RECORDED) == sorted(CASES)


@pytest.mark.parametrize("cid", list(CASES))
def test_dispatch_and_results_match_the_recorded_build(cid, bound, gpu_device):
    lib, Fuse, arenas = bound
    assert CASES[cid](lib, Fuse, arenas, gpu_device) == RECORDED[cid]

"""The optimisation step against a recording of the tree before its host-side state (the Jacobian arena, the persistent zero
gradients, the output-activation link, VQ-VAE-2's lazily formed sums) moved from process-wide registries to the objects that use
it: tests/golden/step_parent.json, written by tests/golden/record_step_parent.py from that tree on an MI355X.  Only host code
changed and the library is the same, so every recorded field must come out the same: the ordered names of the C-ABI calls of
the captured step (the reconstruction loss still applies the output activation's derivative -- movae_recon_loss_bwd_act -- and
VQ-VAE-2 still forms no sums), the deferred-reduce counters of an eager step (the explicit flush before the aggregator moved no
launch) and the SHA-256 of every parameter after three replays.  And any number of captured steps may be alive at once: each
model's arena is its own.  GPU only."""
import gc
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
_spec = importlib.util.spec_from_file_location("record_step_parent", os.path.join(GOLDEN, "record_step_parent.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)
with open(os.path.join(GOLDEN, "step_parent.json")) as _fh:
    RECORDED = json.load(_fh)["cases"]


def test_the_recording_covers_every_case():
    assert sorted(RECORDED) == sorted(rec.TAGS)
    for tag in rec.TAGS:
        assert "movae_recon_loss_bwd_act" in RECORDED[tag]["calls"], tag


@pytest.mark.parametrize("tag", rec.TAGS)
def test_launches_statistics_and_parameters_match_the_recorded_tree(tag, gpu_device):
    import movae_amd  # noqa: F401

    got, want = rec.record(tag, gpu_device), RECORDED[tag]
    assert got["calls"] == want["calls"]
    assert got["defer_stats"] == want["defer_stats"]
    assert got["params"] == want["params"]


def test_zero_gradient_is_allocated_once_on_the_parameter(gpu_device):
    """The bias in front of a training-mode BatchNorm has an identically zero gradient: with no sink registered (a plain
    total_loss.backward()) it is one persistent zero tensor that the PARAMETER keeps -- the same one in the second step."""
    import movae_amd  # noqa: F401

    net, _, x = rec.make("vae_tiny", gpu_device)
    bias, seen = net.encoder[0][0].bias, []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        net.loss_function(x, args=net(x))["total_loss"].backward()
        seen.append(bias._movae_zero_grad.data_ptr())
        assert bias.grad.shape == bias.shape and not bias.grad.any() and not bias._movae_zero_grad.any()
    assert seen[0] == seen[1]


def test_many_live_captured_steps_do_not_disturb_each_other(gpu_device):
    """Five captured steps on five separately built copies of one network, all alive (more than the four arenas the evicting
    cache used to keep): three replays of the FIRST leave its parameters bit for bit where a sixth copy, built and replayed
    alone once the five are gone, ends up -- and where the recorded tree's did."""
    import movae_amd  # noqa: F401

    steps = [rec.graphed_step("vae_tiny", gpu_device) for _ in range(5)]
    arenas = [[a for p in gs.net.parameters() for a in getattr(p, "_movae_j_arenas", ())] for gs, _ in steps]
    assert [len(a) for a in arenas] == [1] * 5 and len({a[0].buf.data_ptr() for a in arenas}) == 5  # one each, on its own model
    first = rec.replayed_params(*steps[0])
    del steps
    gc.collect()
    alone = rec.replayed_params(*rec.graphed_step("vae_tiny", gpu_device))
    assert first == alone
    assert first == RECORDED["vae_tiny"]["params"]

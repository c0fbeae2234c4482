"""Forward launch families under HIP graph replay (stream-ordered, no allocation the caller does not see, no synchronisation, no host
state a result depends on).  tests/test_hip_graph.py checks that for gmpi_mpi_render_launch over float volumes and for the volume backward; here: uint8
volumes in both layouts, float layers in place, the shaded render and the shared-colour layout.  (The table in INTEGRATION.md 4 says which families
have no replay test yet.  These shapes never send AUTO to the band path: no case here touches the lent workspace or the view gate.  The depth-alpha
layout is NOT an ordinary gap: its replay case stopped a GPU session with a HIP error, the cause is not found, and it must not be added again and
run on a GPU before the cause has been found from the code -- see the note under that table.)

One harness (tests/_replay_cases.py `replay`): uncaptured steps on the capture stream give want[i]; one step is recorded after a warm-up; the replays
visit three content sets -- volume AND poses -- in the order A, B, C, B, A with poisoned outputs and zeroed status words.

Bars.  Strict-order mode: the bits of the uncaptured call, and the last replay the bits of oracle.render of the expanded fp32 volume.  Default mode: every
family's own bar against that oracle (colour 0.5e-5, depth and T 1e-5: tests/test_hip_u8_storage.py, test_hip_float_layers.py, test_hip_shaded_render.py,
test_hip_shared_forward_staged.py), and the bits of the uncaptured call where the family's file states bit-equality between two launches of one kernel
in default mode: uint8 volumes (tests/test_hip_u8_occupancy.py, tests/test_hip_u8_interleaved.py) and the one-pixel kernel of the float layers
(tests/test_hip_float_layers.py `check_layers`: default gather == planar gather)."""
import numpy as np
import pytest

import _replay_cases as R

pytestmark = pytest.mark.gpu

KEYS = R.KEYS
# default mode: the families whose own test file states bit-equality between two launches of one kernel
BITS_IN_DEFAULT_MODE = ("u8-planar", "u8-channels-last", "layers-f32-gather", "layers-bf16-gather")
FALLBACK_COUNTERS = ("shared_lds_fallbacks", "shaded_lds_fallbacks", "layers_copies", "layers_lds_fallbacks")


def _forward_compare(box, strict, bits_in_default, label):
    """compare() of a forward case: box["case"] is the case once `build` has run."""
    def compare(i, got, want, last):
        case = box["case"]
        if strict or bits_in_default:
            for k in KEYS:
                assert R.same_bits(got[k], want[k]), (label, i, k, float((got[k] - want[k]).abs().max()))
        if strict and last:
            orc = case.oracle(i)
            for k in KEYS:
                assert np.array_equal(got[k].cpu().numpy(), orc[k]), (label, i, k)
        if not strict:
            ok, errs = R.within_the_bars(got, case.oracle(i))
            print(label, "set", i, "default mode against the oracle:", errs)
            assert ok, (label, i, errs)
    return compare


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "default"])
@pytest.mark.parametrize("name", list(R.FAMILIES))
def test_forward_family_replays_from_a_graph(name, strict):
    box = {}

    def build(dev):
        box["case"] = R.ForwardCase(R.FAMILIES[name], strict, dev)
        return box["case"]

    case = R.replay(build, _forward_compare(box, strict, name in BITS_IN_DEFAULT_MODE, name))
    counts = {k: getattr(case.mpi, k) for k in FALLBACK_COUNTERS}
    assert not any(counts.values()), counts

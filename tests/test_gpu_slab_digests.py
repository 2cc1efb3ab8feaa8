"""The BC and AWAC steps, bit for bit against the commit before the slab-step core (csrc/slab_step.h).  -m gpu.

tests/golden/slab_digests.json holds the sha256 of everything both steps write over the smallest shapes of their
envelopes (tests/slab_digests.py has the list and how the file was recorded: from an export of that commit, built
with its own build.py).  Each unit is recomputed on the current build and compared entry by entry; a mismatch names
the first differing tensor and prints the recorded and the current compiler lines, because another compiler may
legitimately contract or order the same source differently.  Nothing here skips.
"""
import json
import os

import pytest

from tests import slab_digests as sd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "slab_digests.json")) as f:
        return json.load(f)


def test_the_record_is_not_of_this_build(recorded):
    """The digests were recorded on another build than the one under test, over exactly today's units."""
    from iqlpref_amd import _lib
    assert recorded["build_tag"] != _lib.build_tag(), "slab_digests.json was recorded on the code under test"
    assert recorded["steps"] == sd.STEPS and sorted(recorded["digests"]) == sorted(sd.UNITS)


@pytest.mark.parametrize("unit", list(sd.UNITS))
def test_same_bits_as_recorded(recorded, unit):
    want, got = recorded["digests"][unit], sd.UNITS[unit]()
    assert list(got) and sorted(got) == sorted(want), f"{unit}: other entries than recorded"
    differing = [k for k in got if got[k] != want[k]]  # (in the order written: step 1 first)
    if differing:
        print(f"IQLTEST slab-digests {unit}: recorded with {recorded['compiler']!r} at build {recorded['build_tag']}, "
              f"now {sd.compiler_line()!r}")
    assert not differing, (f"{unit}: {len(differing)} of {len(got)} tensors differ from the record, first "
                           f"{differing[0]} (recorded compiler {recorded['compiler']!r}, now {sd.compiler_line()!r})")

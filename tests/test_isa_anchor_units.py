"""tools/isa_barrier_reads.py on the anchor units of YOLOv5 and YOLOv7 (the fused anchor head and the planar decode keep their counters and
wave prefixes in LDS between barriers): no barrier is reached with an LDS read in flight.  Compiled the way tests/test_isa_yolo9_units.py compiles its units,
with the plugins' -ffp-contract=off."""
import os
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_barrier_reads as scan  # noqa: E402

CSRC = os.path.join(ROOT, "tensorrtx_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.parametrize("unit", ["anchor_head", "anchor_decode"])
def test_anchor_units_pass_no_barrier_with_lds_reads_in_flight(unit):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, unit + ".s")
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}",
                               "-ffp-contract=off", "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "plugins", unit + ".hip")],
                              stderr=subprocess.DEVNULL)
        n, bad = scan.scan(out)
        assert n > 0, f"{unit}: no kernel found in the listing"
        assert not bad, f"{unit}: barrier reached with LDS reads in flight in {bad}"

"""tools/isa_barrier_reads.py on the YOLO11 units (the fused attention stages K / V tiles in LDS between barriers; the depthwise kernel
has no LDS): no barrier is reached with an LDS read in flight.  Compiled the way tests/test_isa_barrier_reads.py compiles the conv units."""
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
@pytest.mark.parametrize("unit", ["attention", "conv_dw"])
def test_yolo11_units_pass_no_barrier_with_lds_reads_in_flight(unit):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, unit + ".s")
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}", "-mllvm",
                               "-amdgpu-mfma-vgpr-form", "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "kernels", unit + ".hip")],
                              stderr=subprocess.DEVNULL)
        n, bad = scan.scan(out)
        assert n > 0, f"{unit}: no kernel found in the listing"
        assert not bad, f"{unit}: barrier reached with LDS reads in flight in {bad}"

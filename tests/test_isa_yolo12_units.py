"""tools/isa_barrier_reads.py on the YOLOv12 unit (the MFMA area attention stages K and transposed V chunks in LDS between barriers): no
barrier is reached with an LDS read in flight, and the listing holds the matrix instruction the kernel is written for.  Compiled the way
tests/test_isa_new_units.py compiles the YOLO11 units."""
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
def test_attention_mfma_passes_no_barrier_with_lds_reads_in_flight():
    unit = "attention_mfma"
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, unit + ".s")
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}", "-mllvm",
                               "-amdgpu-mfma-vgpr-form", "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "kernels", unit + ".hip")],
                              stderr=subprocess.DEVNULL)
        n, bad = scan.scan(out)
        assert n > 0, f"{unit}: no kernel found in the listing"
        assert not bad, f"{unit}: barrier reached with LDS reads in flight in {bad}"
        with open(out) as f:
            text = f.read()
        assert "v_mfma_f32_16x16x32_f16" in text
        assert "scratch_" not in text   # no spills

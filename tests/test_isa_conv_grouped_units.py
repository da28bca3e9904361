"""tools/isa_barrier_reads.py on the grouped-convolution unit (kernels/conv_grouped.hip stages the input patch and the output tile in LDS between
barriers): no barrier is reached with an LDS read in flight, no instantiation spills, and the registers and occupancy of every one of the sixteen
instantiations are the ones the table of DESIGN.md states.  Compiled the way tests/test_isa_yolo12_units.py compiles its unit."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_barrier_reads as scan  # noqa: E402

CSRC = os.path.join(ROOT, "tensorrtx_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

# DESIGN.md section 5, "Grouped convolution", "Compiled figures": (taps, Cin_g / 16, units per wave) -> (VGPRs + AGPRs, waves per SIMD)
STATED = {(9, 1, 1): (74, 6), (9, 1, 2): (112, 4), (9, 2, 1): (108, 4), (9, 2, 2): (164, 3),
          (9, 3, 1): (166, 3), (9, 3, 2): (226, 2), (9, 4, 1): (184, 2), (9, 4, 2): (267, 1),
          (1, 1, 1): (53, 8), (1, 1, 2): (64, 8), (1, 2, 1): (53, 8), (1, 2, 2): (64, 8),
          (1, 3, 1): (74, 6), (1, 3, 2): (78, 6), (1, 4, 1): (66, 7), (1, 4, 2): (76, 6)}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_conv_grouped_has_no_scratch_no_read_in_flight_at_a_barrier_and_the_stated_registers():
    unit = "conv_grouped"
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, unit + ".s")
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}", "-mllvm",
                               "-amdgpu-mfma-vgpr-form", "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "kernels", unit + ".hip")],
                              stderr=subprocess.DEVNULL)
        n, bad = scan.scan(out)
        assert n == len(STATED), f"{unit}: {n} kernels in the listing"
        assert not bad, f"{unit}: barrier reached with LDS reads in flight in {bad}"
        with open(out) as f:
            text = f.read()
    assert "v_mfma_f32_16x16x32_f16" in text
    assert "scratch_" not in text   # no spills
    assert set(re.findall(r"\.private_segment_fixed_size: (\d+)", text)) == {"0"}
    got = {}
    for m in re.finditer(r"\.amdhsa_kernel \S*conv_grouped_f16_kernelILi(\d)ELi(\d)ELi(\d)E\S*\n.*?\.end_amdhsa_kernel.*?; NumVgprs: (\d+).*?; NumAgprs: (\d+)"
                         r".*?; Occupancy: (\d+)", text, flags=re.S):
        got[tuple(int(v) for v in m.group(1, 2, 3))] = (int(m.group(4)) + int(m.group(5)), int(m.group(6)))
    assert got == STATED

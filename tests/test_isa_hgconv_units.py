"""tools/isa_barrier_reads.py on the hypergraph-convolution unit (kernels/hgconv.hip stages Q, the tokens of a sub-tile, the softmax weights and G in
LDS between barriers): no barrier is reached with an LDS read in flight.  Compiled the way tests/test_isa_yolo12_units.py compiles its unit."""
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
def test_hgconv_passes_no_barrier_with_lds_reads_in_flight():
    unit = "hgconv"
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, unit + ".s")
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}", "-mllvm",
                               "-amdgpu-mfma-vgpr-form", "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "kernels", unit + ".hip")],
                              stderr=subprocess.DEVNULL)
        n, bad = scan.scan(out)
        assert n >= 10, f"{unit}: {n} kernels in the listing, the chain has ten instantiations"
        assert not bad, f"{unit}: barrier reached with LDS reads in flight in {bad}"

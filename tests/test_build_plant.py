"""Build-level guard (CPU, no GPU needed) of mpcqp_plant_kernel, on one device-only compile of
the library for gfx950 and its kernel-resource-usage remarks, as tests/test_build_predict.py
guards mpcqp_predict_kernel.

The kernel must compile without private memory, without register spills and without LDS (DESIGN
§4.4i: the four legs of a robot meet through DPP moves inside their quad): the record's chunk, the
3 x 3 inverses and the cross products are arrays indexed by unrolled loops, which stay in registers
only while every index is a compile-time constant.

Measured on this build: ScratchSize 0, LDS 0, VGPRs 256 (87 further values kept in accumulation
registers), no vector and no scalar register spilled.  The scalar registers are the tight ones:
the float64 constants of sin, cos and atan2 fill most of the 102, and a launch-wide value held
across the loop beside them is spilled into vector lanes (52 were, before the kernel moved its
constants and output addresses into vector registers)."""
import os
import re
import shutil
import subprocess

import pytest

from mpcqp import build as B


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{remark: value} of mpcqp_plant_kernel."""
    if not os.path.exists(B.HIPCC) and not shutil.which("hipcc"):
        pytest.skip("hipcc not installed")
    cmd = [B.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-c",
           "-I" + os.path.join(B.ROOT, "include"), "-o", str(tmp_path_factory.mktemp("build") / "dev.o"), B.SRC,
           "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    hits, on = {"reset": {}}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            on = (hits if re.search(r"\d+mpcqp_plant_kernelE", m.group(1)) else
                  hits["reset"] if re.search(r"\d+mpcqp_plant_reset_kernelE", m.group(1)) else None)
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[", line)
        if m and on is not None:
            on[m.group(1).strip()] = int(m.group(2))
    assert len(hits) > 1 and hits["reset"], "mpcqp_plant_kernel or mpcqp_plant_reset_kernel is not in the build"
    print(f"\nmpcqp_plant_kernel: {hits}")
    return hits


def test_plant_kernel_has_no_private_memory_and_no_lds(usage):
    assert usage.get("ScratchSize") == 0, usage
    assert usage.get("VGPRs Spill") == 0, usage
    assert usage.get("LDS Size") == 0, usage           # the quad meets in registers


def test_reset_kernel_keeps_its_record_in_registers(usage):
    """mpcqp_plant_reset_kernel builds its 48-word record in a local array under a loop over the
    legs: unrolled, it stays in registers."""
    u = usage["reset"]
    assert u.get("ScratchSize") == 0 and u.get("VGPRs Spill") == 0 and u.get("SGPRs Spill") == 0, u


def test_plant_kernel_has_no_scalar_spills(usage):
    assert usage.get("SGPRs Spill") == 0, usage

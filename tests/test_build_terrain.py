"""Build-level guard (CPU, no GPU needed): mpcqp_terrain_kernel must compile for gfx950
without private memory -- its record, the 3 x 3 matrices of the Jacobi sweeps and its small
vectors are arrays indexed by unrolled loops and template arguments, which stay in registers
only while every index is a compile-time constant.  The recipe is that of
tests/test_build_att.py."""
import os
import re
import shutil
import subprocess

import pytest

from mpcqp import build as B


@pytest.mark.skipif(not os.path.exists(B.HIPCC) and not shutil.which("hipcc"), reason="hipcc not installed")
def test_terrain_kernel_has_no_scratch_and_no_spills(tmp_path):
    cmd = [B.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-c",
           "-I" + os.path.join(B.ROOT, "include"), "-o", str(tmp_path / "dev.o"), B.SRC,
           "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    usage = {}
    name = None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[", line)
        if m and name:
            usage[name][m.group(1).strip()] = int(m.group(2))
    hits = [v for n, v in usage.items() if "mpcqp_terrain_kernel" in n]
    assert len(hits) == 1, sorted(usage)
    u = hits[0]
    print(f"\nmpcqp_terrain_kernel: {u}")
    assert u.get("ScratchSize") == 0, u
    assert u.get("VGPRs Spill") == 0 and u.get("SGPRs Spill") == 0, u
    assert u.get("LDS Size") == 0, u          # one thread per robot: nothing is shared

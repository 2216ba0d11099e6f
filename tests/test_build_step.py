"""Build-level guard (CPU, no GPU needed): the three instantiations of mpcqp_step_kernel --
STEP_WHOLE, STEP_FRONT, STEP_BACK -- must compile for gfx950 without private memory and
without register spills.  The kernel holds 24 pointers and the swing constants; its gains go
through LDS so that the scalar registers suffice.  The recipe is that of
tests/test_build_att.py."""
import os
import re
import shutil
import subprocess

import pytest

from mpcqp import build as B


@pytest.mark.skipif(not os.path.exists(B.HIPCC) and not shutil.which("hipcc"), reason="hipcc not installed")
def test_step_kernels_have_no_scratch_and_no_spills(tmp_path):
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
    hits = {n: v for n, v in usage.items() if "mpcqp_step_kernel" in n}
    assert len(hits) == 3, sorted(usage)
    # the template argument in the mangled name: ILi0E WHOLE, ILi1E FRONT, ILi2E BACK
    modes = {int(re.search(r"mpcqp_step_kernelILi(\d)E", n).group(1)): v for n, v in hits.items()}
    assert sorted(modes) == [0, 1, 2], sorted(hits)
    for mode, u in sorted(modes.items()):
        print(f"\nmpcqp_step_kernel<{('WHOLE', 'FRONT', 'BACK')[mode]}>: VGPRs {u.get('VGPRs')}, "
              f"SGPRs {u.get('TotalSGPRs')}, LDS {u.get('LDS Size')} bytes; {u}")
        assert u.get("ScratchSize") == 0, (mode, u)
        assert u.get("VGPRs Spill") == 0 and u.get("SGPRs Spill") == 0, (mode, u)
        assert 0 < u.get("LDS Size") < 64 * 1024, (mode, u)
    # the horizon rows' staging exists in FRONT alone
    assert modes[1]["LDS Size"] > modes[0]["LDS Size"] == modes[2]["LDS Size"]

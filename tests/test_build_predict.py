"""Build-level guard (CPU, no GPU needed) of mpcqp_predict_kernel, on one device-only compile of
the library for gfx950 and its kernel-resource-usage remarks, as tests/test_build.py guards the
other kernels.

The four instantiations <NM = 16 or 32 stages, FULL weights or not> must compile without private
memory and without register spills: the X entries a lane holds, the 3 x 3 matrices of the
model's head and the six cone slacks are arrays indexed by unrolled loops, which stay in
registers only while every index is a compile-time constant.  Each one's LDS is one
PredictShared<NM, FULL> per workgroup: the launch picks the smallest that holds
its horizon and weights, which decides how many robots a CU holds at once."""
import os
import re
import shutil
import subprocess

import pytest

from mpcqp import build as B


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{(NM, FULL): {remark: value}} of the instantiations of mpcqp_predict_kernel."""
    if not os.path.exists(B.HIPCC) and not shutil.which("hipcc"):
        pytest.skip("hipcc not installed")
    cmd = [B.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-c",
           "-I" + os.path.join(B.ROOT, "include"), "-o", str(tmp_path_factory.mktemp("build") / "dev.o"), B.SRC,
           "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    hits, key = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            # the template arguments in the mangled name: ILi<NM>ELb<FULL>E
            k = re.search(r"mpcqp_predict_kernelILi(\d+)ELb([01])E", m.group(1))
            key = (int(k.group(1)), bool(int(k.group(2)))) if k else None
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[", line)
        if m and key:
            hits.setdefault(key, {})[m.group(1).strip()] = int(m.group(2))
    assert sorted(hits) == [(16, False), (16, True), (32, False), (32, True)], sorted(hits)
    return hits


def test_predict_kernels_have_no_scratch_and_no_spills(usage):
    for key, u in sorted(usage.items()):
        print(f"\nmpcqp_predict_kernel<{key[0]}, {str(key[1]).lower()}>: {u}")
        assert u.get("ScratchSize") == 0, (key, u)
        assert u.get("VGPRs Spill") == 0 and u.get("SGPRs Spill") == 0, (key, u)
        assert u.get("AGPRs") == 0, (key, u)


def test_predict_kernel_lds_holds_its_stages(usage):
    """The staged inputs alone are (44 + 4 NM + 13 NM + 12 NM) floats and the two scans 192 NM
    bytes: under that a layout cannot hold NM stages.  The largest, <32, true>, is the 20 416
    bytes DESIGN §4.4h states (7 workgroups in a CU's 160 KiB); the one the default horizon and
    weights take, <16, false>, lets a CU hold 16 robots and more."""
    for (nm, full), u in usage.items():
        assert 4 * (44 + 29 * nm) + 192 * nm < u.get("LDS Size"), ((nm, full), u)
    assert usage[(32, True)]["LDS Size"] == 20416
    assert usage[(16, False)]["LDS Size"] < usage[(16, True)]["LDS Size"] < usage[(32, True)]["LDS Size"]
    assert usage[(16, False)]["LDS Size"] < usage[(32, False)]["LDS Size"] < usage[(32, True)]["LDS Size"]
    assert 16 * usage[(16, False)]["LDS Size"] <= 160 * 1024
    assert usage[(16, False)]["Occupancy"] >= 4          # 16 one-wave workgroups per CU of 4 SIMDs

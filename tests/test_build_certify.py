"""Build-level guard (CPU, no GPU needed) of mpcqp_certify_kernel, on one device-only compile of
the library for gfx950 and its kernel-resource-usage remarks, as tests/test_build_predict.py
guards mpcqp_predict_kernel.

The four instantiations <NM = 16 or 32 stages, FULL weights or not> must compile without private
memory and without register spills: the G entries a lane holds, the 3 x 3 matrices of the
model's head, the record copy behind the cone frame and a foot-step's gradient are arrays indexed
by unrolled loops, which stay in registers only while every index is a compile-time constant.
Each one's LDS is one CertifyShared<NM, FULL> per workgroup, the size its static_assert states
(csrc/mpcqp_certify.h)."""
import os
import re
import shutil
import subprocess

import pytest

from mpcqp import build as B


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{(NM, FULL): {remark: value}} of the instantiations of mpcqp_certify_kernel."""
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
            k = re.search(r"mpcqp_certify_kernelILi(\d+)ELb([01])E", m.group(1))
            key = (int(k.group(1)), bool(int(k.group(2)))) if k else None
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[", line)
        if m and key:
            hits.setdefault(key, {})[m.group(1).strip()] = int(m.group(2))
    assert sorted(hits) == [(16, False), (16, True), (32, False), (32, True)], sorted(hits)
    return hits


def stated_lds():
    """{(NM, FULL): bytes} from the static_assert of csrc/mpcqp_certify.h."""
    src = open(os.path.join(os.path.dirname(B.SRC), "mpcqp_certify.h")).read()
    found = re.findall(r"sizeof\(CertifyShared<(\w+), (true|false)>\) == (\d+)", src)
    return {(32 if nm == "kMaxN" else int(nm), full == "true"): int(size) for nm, full, size in found}


def test_certify_kernels_have_no_scratch_and_no_spills(usage):
    for key, u in sorted(usage.items()):
        print(f"\nmpcqp_certify_kernel<{key[0]}, {str(key[1]).lower()}>: {u}")
        assert u.get("ScratchSize") == 0, (key, u)
        assert u.get("VGPRs Spill") == 0 and u.get("SGPRs Spill") == 0, (key, u)
        assert u.get("AGPRs") == 0, (key, u)


def test_certify_kernel_lds_is_what_its_static_assert_states(usage):
    stated = stated_lds()
    assert sorted(stated) == sorted(usage)
    for key, u in usage.items():
        assert u.get("LDS Size") == stated[key], (key, u, stated[key])
    assert stated == {(16, False): 9808, (16, True): 15424, (32, False): 18064, (32, True): 27008}
    # the staged inputs, the forward sums and the backward sums alone: under that a layout cannot hold NM stages
    for (nm, full), size in stated.items():
        assert 4 * (44 + 29 * nm) + 192 * nm + 208 * nm < size
    assert 16 * stated[(16, False)] <= 160 * 1024      # 16 robots in a CU at the default horizon and weights
    assert usage[(16, False)]["Occupancy"] >= 4        # 16 one-wave workgroups per CU of 4 SIMDs

"""Build-level guards (CPU, no GPU needed), on one compile of the library for gfx950 and its
kernel-resource-usage remarks.

The dense QP classes must compile without private-memory spills.  A spill in the active-set
loop costs a scratch store/load per pass and shows up as HBM write traffic (a
4-byte VGPR spill once added ~266 KiB of write-back per config-2 launch).

mpcqp_attitude_kernel and mpcqp_terrain_kernel must compile without private memory -- their
records, the 3 x 3 matrices of the terrain's Jacobi sweeps and their small vectors are arrays
indexed by unrolled loops and template arguments, which stay in registers only while every
index is a compile-time constant.

The three instantiations of mpcqp_step_kernel -- STEP_WHOLE, STEP_FRONT, STEP_BACK -- must
compile without private memory and without register spills.  The kernel holds 24 pointers and
the swing constants; its gains go through LDS so that the scalar registers suffice
(DESIGN §4.4f)."""
import os
import re
import shutil
import subprocess

import pytest

from mpcqp import build as B

DENSE = ("mpcqp_kernel_64", "mpcqp_kernel_96", "mpcqp_kernel_128")


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{mangled kernel name: {remark: value}} of one device-only compile."""
    if not os.path.exists(B.HIPCC) and not shutil.which("hipcc"):
        pytest.skip("hipcc not installed")
    cmd = [B.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-c",
           "-I" + os.path.join(B.ROOT, "include"), "-o", str(tmp_path_factory.mktemp("build") / "dev.o"), B.SRC,
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
    return usage


def test_dense_classes_are_spill_free(usage):
    for k in DENSE:
        hits = [v for n, v in usage.items() if k in n]
        assert hits, (k, sorted(usage))
        u = hits[0]
        assert u.get("ScratchSize") == 0, (k, u)
        assert u.get("VGPRs Spill") == 0, (k, u)
        assert u.get("Occupancy") >= 2, (k, u)   # two robots' waves per SIMD


def test_attitude_kernel_has_no_scratch_and_no_spills(usage):
    hits = [v for n, v in usage.items() if "mpcqp_attitude_kernel" in n]
    assert len(hits) == 1, sorted(usage)
    u = hits[0]
    print(f"\nmpcqp_attitude_kernel: {u}")
    assert u.get("ScratchSize") == 0, u
    assert u.get("VGPRs Spill") == 0 and u.get("SGPRs Spill") == 0, u
    assert u.get("LDS Size") == 0, u          # one thread per robot: nothing is shared


def test_step_kernels_have_no_scratch_and_no_spills(usage):
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


def test_terrain_kernel_has_no_scratch_and_no_spills(usage):
    hits = [v for n, v in usage.items() if "mpcqp_terrain_kernel" in n]
    assert len(hits) == 1, sorted(usage)
    u = hits[0]
    print(f"\nmpcqp_terrain_kernel: {u}")
    assert u.get("ScratchSize") == 0, u
    assert u.get("VGPRs Spill") == 0 and u.get("SGPRs Spill") == 0, u
    assert u.get("LDS Size") == 0, u          # one thread per robot: nothing is shared

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
(DESIGN §4.4f).

The four instantiations <NM = 16 or 32 stages, FULL weights or not> of mpcqp_predict_kernel must
compile without private memory and without register spills: the X entries a lane holds, the 3 x 3
matrices of the model's head and the six cone slacks are arrays indexed by unrolled loops, which
stay in registers only while every index is a compile-time constant -- through the rollout_*
functions and the lambdas the kernel hands them as well.  Each one's LDS is one
PredictShared<NM, FULL> per workgroup: the launch picks the smallest that holds
its horizon and weights, which decides how many robots a CU holds at once.

mpcqp_plant_kernel must compile without private memory, without register spills and without LDS
(the four legs of a robot meet through DPP moves inside their quad): the record's
chunk, the 3 x 3 inverses and the cross products are arrays indexed by unrolled loops, which stay
in registers only while every index is a compile-time constant.  Measured on this build:
ScratchSize 0, LDS 0, VGPRs 256 (87 further values kept in accumulation registers), no vector and
no scalar register spilled.  The scalar registers are the tight ones: the float64 constants of
sin, cos and atan2 fill most of the 102, and a launch-wide value held across the loop beside them
is spilled into vector lanes (52 were, before the kernel moved its constants and output addresses
into vector registers).

The four instantiations of mpcqp_certify_kernel, <NM, FULL> as predict's, must compile without
private memory and without register spills: the G entries a lane holds, the 3 x 3 matrices of the
model's head, the record copy behind the cone frame and a foot-step's gradient are arrays indexed
by unrolled loops, which stay in registers only while every index is a compile-time constant.
Each one's LDS is one CertifyShared<NM, FULL> per workgroup, the size its static_assert states
(csrc/mpcqp_certify.h)."""
import os
import re

import pytest

from helpers import kernel_usage
from mpcqp import build as B

DENSE = ("mpcqp_kernel_64", "mpcqp_kernel_96", "mpcqp_kernel_128")


@pytest.fixture(scope="module")
def usage():
    return kernel_usage()


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


def _instantiations(usage, kernel):
    """{(NM, FULL): remarks} of a kernel's four instantiations, by the template arguments in the
    mangled name: ILi<NM>ELb<FULL>E."""
    hits = {}
    for n, v in usage.items():
        k = re.search(kernel + r"ILi(\d+)ELb([01])E", n)
        if k:
            hits[(int(k.group(1)), bool(int(k.group(2))))] = v
    assert sorted(hits) == [(16, False), (16, True), (32, False), (32, True)], sorted(hits)
    return hits


def test_predict_kernels_have_no_scratch_and_no_spills(usage):
    for key, u in sorted(_instantiations(usage, "mpcqp_predict_kernel").items()):
        print(f"\nmpcqp_predict_kernel<{key[0]}, {str(key[1]).lower()}>: {u}")
        assert u.get("ScratchSize") == 0, (key, u)
        assert u.get("VGPRs Spill") == 0 and u.get("SGPRs Spill") == 0, (key, u)
        assert u.get("AGPRs") == 0, (key, u)


def test_predict_kernel_lds_holds_its_stages(usage):
    """The staged inputs alone are (44 + 4 NM + 13 NM + 12 NM) floats and the two scans 192 NM
    bytes: under that a layout cannot hold NM stages.  The largest, <32, true>, is the 20 416
    bytes DESIGN §4.4h states (7 workgroups in a CU's 160 KiB); the one the default horizon and
    weights take, <16, false>, lets a CU hold 16 robots and more."""
    usage = _instantiations(usage, "mpcqp_predict_kernel")
    for (nm, full), u in usage.items():
        assert 4 * (44 + 29 * nm) + 192 * nm < u.get("LDS Size"), ((nm, full), u)
    assert usage[(32, True)]["LDS Size"] == 20416
    assert usage[(16, False)]["LDS Size"] < usage[(16, True)]["LDS Size"] < usage[(32, True)]["LDS Size"]
    assert usage[(16, False)]["LDS Size"] < usage[(32, False)]["LDS Size"] < usage[(32, True)]["LDS Size"]
    assert 16 * usage[(16, False)]["LDS Size"] <= 160 * 1024
    assert usage[(16, False)]["Occupancy"] >= 4          # 16 one-wave workgroups per CU of 4 SIMDs


def _one(usage, kernel):
    """The remarks of a kernel that is no template, by its length-prefixed mangled name."""
    hits = [v for n, v in usage.items() if re.search(r"\d+" + kernel + "E", n)]
    assert len(hits) == 1, (kernel, sorted(usage))
    return hits[0]


def test_plant_kernel_has_no_private_memory_and_no_lds(usage):
    u = _one(usage, "mpcqp_plant_kernel")
    print(f"\nmpcqp_plant_kernel: {u}")
    assert u.get("ScratchSize") == 0, u
    assert u.get("VGPRs Spill") == 0, u
    assert u.get("LDS Size") == 0, u           # the quad meets in registers


def test_reset_kernel_keeps_its_record_in_registers(usage):
    """mpcqp_plant_reset_kernel builds its 48-word record in a local array under a loop over the
    legs: unrolled, it stays in registers."""
    u = _one(usage, "mpcqp_plant_reset_kernel")
    assert u.get("ScratchSize") == 0 and u.get("VGPRs Spill") == 0 and u.get("SGPRs Spill") == 0, u


def test_plant_kernel_has_no_scalar_spills(usage):
    u = _one(usage, "mpcqp_plant_kernel")
    assert u.get("SGPRs Spill") == 0, u


def stated_lds():
    """{(NM, FULL): bytes} from the static_assert of csrc/mpcqp_certify.h."""
    src = open(os.path.join(os.path.dirname(B.SRC), "mpcqp_certify.h")).read()
    found = re.findall(r"sizeof\(CertifyShared<(\w+), (true|false)>\) == (\d+)", src)
    return {(32 if nm == "kMaxN" else int(nm), full == "true"): int(size) for nm, full, size in found}


def test_certify_kernels_have_no_scratch_and_no_spills(usage):
    for key, u in sorted(_instantiations(usage, "mpcqp_certify_kernel").items()):
        print(f"\nmpcqp_certify_kernel<{key[0]}, {str(key[1]).lower()}>: {u}")
        assert u.get("ScratchSize") == 0, (key, u)
        assert u.get("VGPRs Spill") == 0 and u.get("SGPRs Spill") == 0, (key, u)
        assert u.get("AGPRs") == 0, (key, u)


def test_certify_kernel_lds_is_what_its_static_assert_states(usage):
    usage = _instantiations(usage, "mpcqp_certify_kernel")
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

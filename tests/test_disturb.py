"""CPU: the sensor model and the push (mpcqp_sensors, mpcqp_push) without a GPU -- the ABI and
Python surface, the generator's known answers, the per-robot header csrc/mpcqp_sensors_robot.h
compiled with g++ and driven through ctypes against the restatement tests/disturb_ref.py, the
statistics of the restatement's draws, quantisation, touch lag and dropout, the identity, the
push's physics, the sensed closed loop on the CPU oracles against its recorded figures
(tests/golden/disturb_loop.npz), and the kernels' resource remarks on one device-only compile.

mpcqp_set_sensors needs a context, which needs a device: its refusals are checked in
tests/test_gpu_disturb.py.

Measured here (printed by the tests):
  header against restatement, 50 ticks, B = 1, 3, 4, 5, 17: integers bitwise; bias words differ
    by 0 and no float32 word differs (log, sin and cos are spelled out in IEEE operations on
    both sides), held to HEADER_BIAS_BOUND = 0
  mpcqp_sensors_kernel: ScratchSize 0, no vector or scalar register spilled, LDS 0, 58 VGPRs
  mpcqp_push_kernel:    ScratchSize 0, no register spilled, LDS 0
"""
import os
import re

import numpy as np
import pytest

import disturb_ref as dr
import plant_ref as pr
from helpers import _vp, host_build, kernel_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mpcqp_disturb_abi.h")
# The worst difference of a bias word between the g++-compiled header and the restatement,
# measured here: 0.  Both evaluate log, sin and cos by the same IEEE operations in the same order
# (sense_log, sense_sincos_turn), and sqrt, / and rint are correctly rounded on both sides.
HEADER_BIAS_BOUND = 0.0

SHIM = r'''
#include "mpcqp_sensors_robot.h"
// a launch of mpcqp_sensors_kernel, robot after robot; ip: key0, key1, drop, touch_lag;
// dp: sigma_gyro, sigma_accel, walk_gyro, walk_accel, bias0_gyro, bias0_accel, sigma_q, sigma_qd, q_lsb, sqrt_dt
extern "C" void sensors(int B, const unsigned* ip, const double* dp, const float* gyro, const float* accel,
                        const float* dofs, const float* touch, const float* scale, double* state, float* gyro_m,
                        float* accel_m, float* dofs_m, float* touch_m, int* status) {
  SenseParams P{ip[0], ip[1], dp[0], dp[1], dp[2], dp[3], dp[4], dp[5], dp[6], dp[7], dp[8], dp[9], ip[2], (int)ip[3]};
  for (size_t b = 0; b < (size_t)B; ++b) {
    const int st = sense_robot(P, state + SENSE_STRIDE * b, gyro ? gyro + 3 * b : nullptr, accel ? accel + 3 * b : nullptr,
                               dofs ? dofs + 24 * b : nullptr, touch ? touch + 4 * b : nullptr, scale ? scale + b : nullptr,
                               gyro_m ? gyro_m + 3 * b : nullptr, accel_m ? accel_m + 3 * b : nullptr,
                               dofs_m ? dofs_m + 24 * b : nullptr, touch_m ? touch_m + 4 * b : nullptr);
    if (status) status[b] = st;
  }
}
extern "C" void philox(const unsigned* c, const unsigned* k, unsigned* out) { sense_philox(c[0], c[1], c[2], c[3], k[0], k[1], out); }
extern "C" void normals(unsigned w0, unsigned w1, double* z) { sense_normals(w0, w1, z, z + 1); }
extern "C" void push(int B, const float* impulse, const float* point, const float* robot, double* state, int* status) {
  for (size_t b = 0; b < (size_t)B; ++b)
    status[b] = push_robot(state + PLANT_STRIDE * b, impulse + 3 * b, point ? point + 3 * b : impulse, point != nullptr,
                           robot + 16 * b);
}
extern "C" int stride(void) { return SENSE_STRIDE; }
extern "C" int words(void) { return SENSE_WORDS; }
'''


@pytest.fixture(scope="module")
def header():
    return host_build(SHIM, ("-O2", "-std=c++17", "-ffp-contract=off"), "disturb")


def run_header(header, state, P, gyro=None, accel=None, dofs=None, touch=None, scale=None):
    """disturb_ref.tick's call through the host-compiled header: in place on state."""
    B = len(state)
    f4 = np.float32
    ins = [None if v is None else np.ascontiguousarray(v, f4) for v in (gyro, accel, dofs, touch)]
    outs = [None if v is None else np.full_like(v, -7.0) for v in ins]
    ip = np.array([P.seed & 0xFFFFFFFF, P.seed >> 32, int(np.floor(P.p_drop * 2.0 ** 32)), P.touch_lag], np.uint32)
    dp = np.array([P.sigma_gyro, P.sigma_accel, P.walk_gyro, P.walk_accel, P.bias0_gyro, P.bias0_accel, P.sigma_q,
                   P.sigma_qd, P.q_lsb, np.sqrt(P.dt)], np.float64)
    status = np.full(B, -3, np.int32)
    sc = None if scale is None else np.ascontiguousarray(scale, f4)
    header.sensors(B, _vp(ip), _vp(dp), *map(_vp, ins), _vp(sc), _vp(state), *map(_vp, outs), _vp(status))
    out = {k: v for k, v in zip(("gyro", "accel", "dofs", "touch"), outs) if v is not None}
    if "dofs" in out:
        out["dofs"] = out["dofs"].reshape(B, 12, 2)
    out["status"] = status
    return out


def plant_like(rng, B):
    """Inputs of the plant's shapes and magnitudes; touch 0 / 1."""
    f4 = np.float32
    return dict(gyro=rng.normal(0, 0.3, (B, 3)).astype(f4), accel=(rng.normal(0, 1.0, (B, 3)) + [0, 0, 9.81]).astype(f4),
                dofs=rng.normal(0, 1.0, (B, 12, 2)).astype(f4), touch=(rng.random((B, 4)) < 0.6).astype(f4))


# ---- the ABI and Python surface

def test_constants_agree(header):
    from mpcqp import _lib
    from mpcqp import sensors
    src = open(HEADER).read()
    assert int(re.search(r"#define MPCQP_SENSE_STRIDE (\d+)", src).group(1)) == _lib.SENSE_STRIDE == dr.STRIDE == header.stride() == 16
    assert header.words() == dr.WORDS == 13
    assert (dr.STATUS_OK, dr.STATUS_NONFINITE) == (_lib.STATUS_OK, _lib.STATUS_NONFINITE)
    assert sensors.SENSOR_PRESETS["mems"] == dr.MEMS
    assert (sensors._BIAS_G, sensors._BIAS_A, sensors._INIT, sensors._COUNT, sensors._ID, sensors._HIST) == \
        (dr.BIAS_G, dr.BIAS_A, dr.INIT, dr.COUNT, dr.ID, dr.HIST)


def test_null_ctx_is_an_error_code():
    from mpcqp import _lib
    lib = _lib.load()
    assert lib.mpcqp_sensors(None, 1, 0, *([None] * 12)) == -1
    assert lib.mpcqp_set_sensors(None, 0, *([0.0] * 9), 0, 0.0) == -1
    assert lib.mpcqp_push(None, 1, *([None] * 6)) == -1


def test_python_surface():
    import mpcqp
    from mpcqp.plant import BatchedPlant
    from mpcqp.sensors import SENSOR_PRESETS, BatchedSensors
    assert "BatchedSensors" in mpcqp.__all__ and mpcqp.BatchedSensors is BatchedSensors
    assert mpcqp.SENSOR_PRESETS is SENSOR_PRESETS
    for name in ("update", "bind_update", "reset", "set_constants"):
        assert getattr(BatchedSensors, name).__doc__
    for name in ("bias_gyro", "bias_accel", "count", "status", "history"):
        assert isinstance(getattr(BatchedSensors, name), property)
    assert BatchedPlant.push.__doc__ and BatchedPlant.bind_push.__doc__
    assert "not measurements" in BatchedSensors.__doc__


# ---- the generator

def test_known_answers(header):
    """The three vectors of the generator's definition, through the restatement and the header."""
    for ctr, key, want in dr.KNOWN:
        assert dr.philox(np.array(ctr, np.uint64), np.array(key, np.uint64)).tolist() == list(want)
        out = np.zeros(4, np.uint32)
        header.philox(_vp(np.array(ctr, np.uint32)), _vp(np.array(key, np.uint32)), _vp(out))
        assert out.tolist() == list(want)


def test_normals_of_extreme_words(header):
    """|z| <= 6.77 at the smallest u0, and the header's Box-Muller agrees with the restatement."""
    worst = 0.0
    for w0, w1 in ((0, 0), (0, 0xFFFFFFFF), (0xFFFFFFFF, 0), (0x80000000, 0x40000000), (12345, 0xC0000000)):
        z = np.zeros(2)
        header.normals(w0, w1, _vp(z))
        a, b = dr.normals(np.array([w0], np.uint32), np.array([w1], np.uint32))
        assert np.abs(z).max() <= 6.77 and np.isfinite(z).all()
        worst = max(worst, abs(z[0] - a[0]), abs(z[1] - b[0]))
    assert worst == 0.0, worst


# ---- the header against the restatement

@pytest.mark.parametrize("B", (1, 3, 4, 5, 17))
def test_header_against_restatement(header, B):
    """T = 50 ticks of the preset at per-robot scales, dropout on: histories, count, touch_m and
    status bitwise; bias words within HEADER_BIAS_BOUND (measured: 0, which is the bound); float32
    outputs equal."""
    T = 50
    P = dr.Params(seed=0x1234567890ABCDEF, **dict(dr.MEMS, sigma_q=1e-3, p_drop=0.25))
    rng = np.random.default_rng(B)
    scale = (np.arange(B) % 5).astype(np.float32)
    a, b = dr.new_state(B), dr.new_state(B)
    worst = flips = 0
    for t in range(T):
        ins = plant_like(rng, B)
        ra, rb = dr.tick(a, P, scale=scale, **ins), run_header(header, b, P, scale=scale, **ins)
        assert np.array_equal(a[:, dr.INIT:], b[:, dr.INIT:]), t
        assert np.array_equal(ra["touch"], rb["touch"]) and np.array_equal(ra["status"], rb["status"])
        worst = max(worst, np.abs(a[:, :6] - b[:, :6]).max())
        for k in ("gyro", "accel", "dofs"):
            d = ra[k] != rb[k]
            flips += int(d.sum())
            lim = np.maximum(np.spacing(np.abs(ra[k])), np.float32(P.q_lsb * 1.0001) if k == "dofs" else 0)
            assert (np.abs(ra[k].astype(np.float64) - rb[k]) <= lim)[d].all(), (t, k)
    print(f"\nB = {B}: worst bias difference {worst:.3e}, float32 words differing {flips}")
    assert (a[:, dr.COUNT] == T).all() and flips == 0
    assert worst <= HEADER_BIAS_BOUND


def test_refusals_in_the_header_and_the_restatement(header):
    """One robot per cause is refused with its record untouched and its outputs its inputs; the
    others draw what they draw without it."""
    B = 10
    P = dr.Params(seed=3, **dr.MEMS)
    rng = np.random.default_rng(0)
    ins = plant_like(rng, B)
    scale = np.ones(B, np.float32)
    st = dr.new_state(B)
    dr.tick(st, P, scale=scale, **ins)                      # initialised records
    clean = st.copy()
    want = dr.tick(clean, P, scale=scale, **ins)
    bad_in = {k: v.copy() for k, v in ins.items()}
    bad_in["gyro"][0, 1] = np.nan
    bad_in["dofs"][1, 7, 1] = np.inf
    bad_in["touch"][2, 3] = np.nan
    bad_scale = scale.copy()
    bad_scale[3], bad_scale[4] = np.nan, -1.0
    st0 = st.copy()
    st0[5, dr.HIST + 2] = np.nan
    st0[6, dr.COUNT], st0[7, dr.ID] = -1.0, 2.0 ** 32          # outside the integers they are read as
    for run in (lambda s: dr.tick(s, P, scale=bad_scale, **bad_in), lambda s: run_header(header, s, P, scale=bad_scale, **bad_in)):
        s = st0.copy()
        out = run(s)
        assert out["status"].tolist() == [4] * 8 + [0] * 2
        assert np.array_equal(s[:8].view(np.uint64), st0[:8].view(np.uint64))
        assert np.array_equal(s[8:], clean[8:])
        for k in ("gyro", "accel", "dofs", "touch"):
            assert np.array_equal(out[k][:8].view(np.uint32), bad_in[k][:8].view(np.uint32)), k
            assert np.array_equal(out[k][8:], want[k][8:]), k


def test_null_groups_do_not_change_the_draws(header):
    B, P = 5, dr.Params(seed=9, **dr.MEMS)
    ins = plant_like(np.random.default_rng(1), B)
    for run in (dr.tick, lambda s, P, **kw: run_header(header, s, P, **kw)):
        full_state = dr.new_state(B)
        full = [run(full_state, P, **ins) for _ in range(3)][-1]
        for left_out in ("gyro", "accel", "dofs"):
            s = dr.new_state(B)
            part = {k: v for k, v in ins.items() if k != left_out}
            out = [run(s, P, **part) for _ in range(3)][-1]
            assert np.array_equal(s, full_state) and left_out not in out
            for k in part:
                assert np.array_equal(out[k], full[k]), (left_out, k)
        s = dr.new_state(B)                                  # without touch the histories stay
        out = [run(s, P, **{k: v for k, v in ins.items() if k != "touch"}) for _ in range(3)][-1]
        assert np.array_equal(s[:, :dr.HIST], full_state[:, :dr.HIST]) and (s[:, dr.HIST:dr.HIST + 4] == 0).all()
        assert np.array_equal(out["gyro"], full["gyro"]) and np.array_equal(out["dofs"], full["dofs"])


# ---- statistics of the restatement

def test_moments_of_the_restatement():
    """64 robots x 200 ticks, seeded: all sigmas and walks 1, dt 1, inputs zero, so that the 36
    normals of a robot and tick are read off the outputs (24 joint channels, 3 + 3 white, 3 + 3
    walk increments).  Mean within 5 / sqrt(n), variance within 5 sqrt(2 / n), the correlation
    of any two channels and of a channel between robots id and id + 1 below 5 / sqrt(n); the
    walk's variance after T ticks is walk^2 dt T within the same bound on its 64 x 6 samples."""
    B, T = 64, 200
    P = dr.Params(seed=2026, sigma_gyro=1, sigma_accel=1, walk_gyro=1, walk_accel=1, sigma_q=1, sigma_qd=1, dt=1.0)
    st = dr.new_state(B)
    z = np.zeros((T, B, 36))
    zero = dict(gyro=np.zeros((B, 3), np.float32), accel=np.zeros((B, 3), np.float32), dofs=np.zeros((B, 12, 2), np.float32))
    for t in range(T):
        before = st[:, :6].copy()
        out = dr.tick(st, P, **zero)
        z[t, :, :24] = out["dofs"].reshape(B, 24)
        z[t, :, 24:27] = out["gyro"] - st[:, 0:3]
        z[t, :, 27:30] = out["accel"] - st[:, 3:6]
        z[t, :, 30:36] = st[:, :6] - before
    assert (z[0, :, 30:] == 0).all()                         # no turn-on bias, and no walk on the first call
    white, walk = z[:, :, :30].reshape(-1, 30), z[1:, :, 30:].reshape(-1, 6)
    for x in (white, walk):
        n = len(x)
        assert np.abs(x.mean(0)).max() <= 5 / np.sqrt(n)
        assert np.abs(x.var(0) - 1).max() <= 5 * np.sqrt(2 / n)
    x = z[1:].reshape(-1, 36)
    n = len(x)
    c = np.corrcoef(x.T) - np.eye(36)
    assert np.abs(c).max() <= 5 / np.sqrt(n), np.abs(c).max()
    a, b = z[1:, :-1].reshape(-1, 36), z[1:, 1:].reshape(-1, 36)
    cn = [np.corrcoef(a[:, k], b[:, k])[0, 1] for k in range(36)]
    assert np.abs(cn).max() <= 5 / np.sqrt(len(a)), np.abs(cn).max()
    final = st[:, :6].reshape(-1)
    assert abs(final.var() / (T - 1) - 1) <= 5 * np.sqrt(2 / len(final))
    assert np.abs(z).max() <= 6.77


def test_turn_on_bias_and_scale():
    """The first call draws b = s bias0 z; a robot's scale multiplies sigma, walk and bias0 and
    leaves q_lsb, touch_lag and p_drop alone; scale 0 is the identity but for the quantisation."""
    B = 4096
    P = dr.Params(seed=5, bias0_gyro=0.01, bias0_accel=0.1)
    st = dr.new_state(B)
    dr.tick(st, P)
    n = 3 * B
    assert abs(st[:, 0:3].std() / 0.01 - 1) <= 5 / np.sqrt(2 * n) and abs(st[:, 3:6].std() / 0.1 - 1) <= 5 / np.sqrt(2 * n)
    P = dr.Params(seed=5, **dr.MEMS)
    ins = plant_like(np.random.default_rng(2), 6)
    one, two = dr.new_state(6), dr.new_state(6)
    o1, o2 = dr.tick(one, P, scale=np.ones(6), **ins), dr.tick(two, P, scale=np.full(6, 2.0), **ins)
    assert np.array_equal(two[:, :6], 2 * one[:, :6])
    assert np.allclose(o2["dofs"][..., 1] - ins["dofs"][..., 1], 2 * (o1["dofs"][..., 1] - ins["dofs"][..., 1]), atol=1e-6)
    off = dr.new_state(6)
    o0 = dr.tick(off, P, scale=np.zeros(6), **ins)
    assert (off[:, :6] == 0).all() and np.array_equal(o0["gyro"], ins["gyro"]) and np.array_equal(o0["accel"], ins["accel"])
    assert np.array_equal(o0["dofs"][..., 1], ins["dofs"][..., 1]) and not np.array_equal(o0["dofs"][..., 0], ins["dofs"][..., 0])


def test_quantisation_lands_on_the_grid(header):
    B = 64
    lsb = 2 * np.pi / 2 ** 14
    P = dr.Params(seed=1, sigma_q=2e-3, q_lsb=lsb)
    ins = plant_like(np.random.default_rng(3), B)
    for run in (dr.tick, lambda s, P, **kw: run_header(header, s, P, **kw)):
        q = run(dr.new_state(B), P, dofs=ins["dofs"])["dofs"][..., 0].astype(np.float64)
        k = np.rint(q / lsb)
        assert np.abs(q - k * lsb).max() <= np.spacing(np.float32(np.abs(q).max())) / 2     # one float32 rounding off the grid
        assert np.array_equal((k * lsb).astype(np.float32), q.astype(np.float32))
        assert 0 < np.abs(q - ins["dofs"][..., 0]).max() < 6.77 * 2e-3 + lsb


@pytest.mark.parametrize("lag", (0, 1, 31))
def test_touch_lag_delays_each_edge_exactly(header, lag):
    """A foot's reading at tick t is its input at tick t - lag; before the first `lag` ticks it is
    the first input (the start makes no edges)."""
    B, T = 3, 80
    rng = np.random.default_rng(lag)
    seq = (rng.random((T, B, 4)) < 0.5).astype(np.float32)
    seq[:, 0] = np.repeat(np.arange(T // 8) % 2, 8)[:, None]               # clean square waves on robot 0
    P = dr.Params(seed=4, touch_lag=lag)
    for run in (dr.tick, lambda s, P, **kw: run_header(header, s, P, **kw)):
        st = dr.new_state(B)
        for t in range(T):
            got = run(st, P, touch=seq[t] * (0.3 if t % 2 else 1.0))["touch"]   # any value > 0 is contact
            assert np.array_equal(got, seq[max(t - lag, 0)]), (lag, t)


def test_dropout_rate(header):
    B, T, p = 64, 50, 0.25
    P = dr.Params(seed=77, p_drop=p)
    on = np.ones((B, 4), np.float32)
    for run in (dr.tick, lambda s, P, **kw: run_header(header, s, P, **kw)):
        st = dr.new_state(B)
        got = np.stack([run(st, P, touch=on)["touch"] for _ in range(T)])
        n = got.size
        assert abs((got == 0).mean() - p) <= 5 * np.sqrt(p * (1 - p) / n)
        assert (st[:, dr.HIST:dr.HIST + 4] == 2.0 ** 32 - 1).all()      # a dropped reading is not a lost contact: the history keeps it


def test_all_constants_zero_is_the_identity(header):
    """Outputs equal inputs bit by bit (a negative zero included); touch is 0 / 1 of touch > 0."""
    B = 9
    ins = plant_like(np.random.default_rng(4), B)
    ins["gyro"][0, 0], ins["dofs"][1, 2, 0] = -0.0, -0.0
    for run in (dr.tick, lambda s, P, **kw: run_header(header, s, P, **kw)):
        st = dr.new_state(B)
        for t in range(3):
            out = run(st, dr.Params(seed=11), **ins)
            for k in ins:
                assert np.array_equal(out[k].view(np.uint32), ins[k].view(np.uint32)), k
        assert (st[:, :6] == 0).all() and (st[:, dr.COUNT] == 3).all() and (st[:, dr.INIT] == 1).all()


def test_count_crossing_2_to_32(header):
    B = 3
    P = dr.Params(seed=8, **dr.MEMS)
    ins = plant_like(np.random.default_rng(5), B)
    a = dr.new_state(B)
    a[:, dr.COUNT], a[:, dr.INIT] = 2.0 ** 32 - 2, 1.0
    b = a.copy()
    seen = []
    for t in range(4):
        ra, rb = dr.tick(a, P, **ins), run_header(header, b, P, **ins)
        assert np.array_equal(ra["dofs"], rb["dofs"]) and np.array_equal(a[:, dr.INIT:], b[:, dr.INIT:])
        seen.append(ra["dofs"].copy())
    assert (a[:, dr.COUNT] == 2.0 ** 32 + 2).all()
    assert not np.array_equal(seen[0], seen[2]) and not np.array_equal(seen[1], seen[3])


# ---- the push

def push_states(B, seed):
    st = pr.make_states(B, seed=seed)
    rng = np.random.default_rng(seed)
    J = rng.normal(0, 3.0, (B, 3)).astype(np.float32)
    r = rng.normal(0, 0.2, (B, 3)).astype(np.float32)
    return st["rec"].copy(), st["robot"], J, r


def run_push(header, rec, J, robot, point=None):
    status = np.full(len(rec), -3, np.int32)
    header.push(len(rec), _vp(np.ascontiguousarray(J, np.float32)), _vp(None if point is None else np.ascontiguousarray(point, np.float32)),
                _vp(np.ascontiguousarray(robot, np.float32)), _vp(rec), _vp(status))
    return status


def test_push_obeys_the_momentum_balance(header):
    """m dv = J and I_w dw = (Rq r) x J to a few ulp of the terms; nothing but velocity and rate
    is written; the header agrees with the restatement to rounding."""
    B = 40
    rec0, robot, J, r = push_states(B, 0)
    m = robot[:, 0].astype(np.float64)
    I = pr.inertia(robot)
    for run in (lambda rec: dr.push(rec, J, robot, r), lambda rec: run_push(header, rec, J, robot, r)):
        rec = rec0.copy()
        assert (run(rec) == 0).all()
        keep = np.ones(pr.STRIDE, bool)
        keep[pr.VEL:pr.OMEGA + 3] = False
        assert np.array_equal(rec[:, keep].view(np.uint64), rec0[:, keep].view(np.uint64))
        dv, dw = rec[:, pr.VEL:pr.VEL + 3] - rec0[:, pr.VEL:pr.VEL + 3], rec[:, pr.OMEGA:pr.OMEGA + 3] - rec0[:, pr.OMEGA:pr.OMEGA + 3]
        Jd = J.astype(np.float64)
        vmax = np.abs(rec0[:, pr.VEL:pr.VEL + 3]).max(1, keepdims=True) + np.abs(dv).max(1, keepdims=True)
        assert (np.abs(m[:, None] * dv - Jd) <= 4 * np.spacing(m[:, None] * vmax)).all()
        Rq = pr._rot(rec0[:, pr.QUAT:pr.QUAT + 4])
        Iw = Rq @ I @ Rq.transpose(0, 2, 1)
        t = np.cross(pr._mv(Rq, r.astype(np.float64)), Jd)
        lhs = pr._mv(Iw, dw)
        size = np.abs(Iw).max((1, 2))[:, None] * (np.abs(rec0[:, pr.OMEGA:pr.OMEGA + 3]).max(1, keepdims=True) + np.abs(dw).max(1, keepdims=True))
        assert (np.abs(lhs - t) <= 64 * np.spacing(size) * np.linalg.cond(I)[:, None]).all()
    a, b = rec0.copy(), rec0.copy()
    dr.push(a, J, robot, r), run_push(header, b, J, robot, r)
    assert pr.record_error(b, a).max() <= 7.3e-15


def test_push_zero_and_centre_of_mass_are_bitwise(header):
    B = 16
    rec0, robot, J, r = push_states(B, 1)
    rec0[0, pr.VEL], rec0[1, pr.OMEGA + 2] = -0.0, -0.0
    for run in (lambda rec, J, p: dr.push(rec, J, robot, p), lambda rec, J, p: run_push(header, rec, J, robot, p)):
        for zero in (np.zeros_like(J), -np.zeros_like(J)):
            for p in (None, r):
                rec = rec0.copy()
                assert (run(rec, zero, p) == 0).all() and np.array_equal(rec.view(np.uint64), rec0.view(np.uint64))
        rec = rec0.copy()
        run(rec, J, None)                                     # at the centre of mass the rate is not written
        assert np.array_equal(rec[:, pr.OMEGA:].view(np.uint64), rec0[:, pr.OMEGA:].view(np.uint64))
        assert not np.array_equal(rec[:, pr.VEL:pr.VEL + 3], rec0[:, pr.VEL:pr.VEL + 3])


def test_push_refusals(header):
    """A non-finite impulse or point, a non-finite record word, a non-positive mass, a singular
    inertia, a zero quaternion: STATUS_NONFINITE and the record untouched; the others pushed."""
    B = 8
    rec0, robot, J, r = push_states(B, 2)
    robot, J, r = robot.copy(), J.copy(), r.copy()
    J[0, 1] = np.nan
    r[1, 2] = np.inf
    rec0[2, pr.FEET + 5] = np.nan
    robot[3, 0] = 0.0
    robot[4, 1:7] = 0.0
    rec0[5, pr.QUAT:pr.QUAT + 4] = 0.0
    want = rec0.copy()
    assert dr.push(want, J, robot, r).tolist() == [4] * 6 + [0, 0]
    got = rec0.copy()
    assert run_push(header, got, J, robot, r).tolist() == [4] * 6 + [0, 0]
    for rec in (want, got):
        assert np.array_equal(rec[:6].view(np.uint64), rec0[:6].view(np.uint64))
        assert not np.array_equal(rec[6:], rec0[6:])
    assert pr.record_error(got[6:], want[6:]).max() <= 7.3e-15


# ---- the sensed closed loop on the CPU oracles

def test_sensed_closed_loop_against_its_recorded_figures():
    """disturb_ref.closed_loop_sensed (Aliengo, TROTTING10, 0.5 m/s, N = 10, 600 ticks after the
    50-tick settle): scales 0, 1, 2, 4 of the preset, and lateral impulses 0, 2, 4, 8 N s (and 1 N s)
    at the centre of mass at tick 400 of a noise-free robot.  A fresh run gives the figures of
    tests/golden/disturb_loop.npz (make_golden_disturb.py), to gait_switch.npz's tolerances.

    Recorded: the preset holds at every scale (no halving) -- worst height error 0.0235 m at all
    four, roll 0.032 / 0.036 / 0.029 / 0.042 rad, pitch 0.034 / 0.026 / 0.030 / 0.048 rad, speed
    0.550 / 0.542 / 0.542 / 0.580 m/s, estimate error 5.5 / 5.5 / 5.5 / 13.8 mm.  A shove of 1 or
    2 N s stays within the sensing-chain bounds (roll 0.032, 0.061 rad); 4 and 8 N s do not (roll
    0.126 and 0.292 rad, still growing at the end: the plant pins the stance feet and the body
    keeps its sideways momentum), so 2 N s is the largest that recovers."""
    fx = dict(np.load(os.path.join(ROOT, "tests", "golden", "disturb_loop.npz")))
    assert fx["scales"].tolist() == list(dr.LOOP_SCALES) and fx["pushes"].tolist() == list(dr.LOOP_PUSHES)
    assert fx["preset"].tolist() == [dr.MEMS[k] for k in sorted(dr.MEMS)]
    assert set(dr.LOOP_SCALES[:4]) == {0, 1, 2, 4} and {0, 2, 4, 8} <= set(dr.LOOP_PUSHES)
    run = dr.closed_loop_sensed()
    fig = dr.loop_figures(run["body"], run["est"], run["ok"])
    for k in dr.FIGURES:
        print(f"{k}: {fig[k]}")
    assert run["ok"].all() and np.isfinite(run["body"]).all()
    assert np.abs(fig["height"] - fx["height"]).max() < 5e-5 and np.abs(fig["est_error"] - fx["est_error"]).max() < 5e-5
    for k in ("roll", "pitch", "speed"):
        assert np.abs(fig[k] - fx[k]).max() < 5e-4, k
    assert np.array_equal(fig["within"], fx["within"]) and np.array_equal(fig["recovered"], fx["recovered"])
    assert fig["within"][:4].all()                           # the preset holds at scale 1: it is not halved
    assert fig["within"].tolist() == [True] * 6 + [False, False, True]


# ---- the kernels' resources

@pytest.fixture(scope="module")
def usage():
    return kernel_usage()


@pytest.mark.parametrize("kernel", ("mpcqp_sensors_kernel", "mpcqp_push_kernel"))
def test_kernels_have_no_private_memory_no_spills_and_no_lds(usage, kernel):
    hits = [v for n, v in usage.items() if re.search(r"\d+" + kernel + "E", n)]
    assert len(hits) == 1, sorted(usage)
    u = hits[0]
    print(f"\n{kernel}: {u}")
    assert u.get("ScratchSize") == 0, u
    assert u.get("VGPRs Spill") == 0 and u.get("SGPRs Spill") == 0, u
    assert u.get("LDS Size") == 0, u          # the robot's vote is a ballot, not a barrier
    if kernel == "mpcqp_sensors_kernel":
        assert u.get("Occupancy") >= 4, u     # a 256-thread workgroup is one wavefront per SIMD

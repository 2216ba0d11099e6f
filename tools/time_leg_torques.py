"""Launch times of mpcqp_plan (flags 0), mpcqp_stance_torques and mpcqp_leg_torques at
B = 1024 / 8192: warm, 3000 back-to-back launches per sample between HIP
events, the kernels alternated; then each kernel 100 times in a captured graph (the
device-side cost of a launch without the host's enqueue).  Prints one JSON object.

  python tools/time_leg_torques.py
"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pympc-quadruped_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import swing_ref
from mpcqp import LinearMpc
from mpcqp._lib import PLAN_STRIDE
from mpcqp.params import gait_record

DEV = "cuda:0"
def dev(a, dt=None):
    t = torch.as_tensor(np.ascontiguousarray(a)).to(DEV)
    return (t.to(dt) if dt is not None else t).contiguous()

def timeit(fn, n=3000, warm=300, reps=5):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n): fn()
        b.record(); torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / n)
    return out

res = {}
eng = LinearMpc(horizon=16, robot="aliengo", device=DEV)
for B in (1024, 8192):
    inp = swing_ref.make_inputs(B, 1, seed=B)
    rs = dev(swing_ref.root_states(inp["quat"], inp["pos"], inp["vel"])[0])
    vb, yr = dev(inp["v_body"], torch.float64), dev(inp["yaw_rate"], torch.float64)
    names = ["trot10", "pace10", "trot16", "jump16"]
    gait = dev(np.stack([gait_record(names[b % 4]) for b in range(B)]), torch.int32)
    th, jac, u0 = dev(inp["thighs"]), dev(inp["jac"]), dev(inp["u0"])
    pf, fpb, fvb = dev(inp["pos_feet"][0]), dev(inp["foot_pos_base"][0]), dev(inp["foot_vel_base"][0])
    plan = torch.zeros((B, PLAN_STRIDE), dtype=torch.float64, device=DEV)
    x0 = torch.zeros((B, 13), device=DEV)
    mem = torch.zeros((B, 32), dtype=torch.float64, device=DEV)
    tau = torch.zeros((B, 12), device=DEV)
    tick = torch.full((B,), 130, dtype=torch.int32, device=DEV)   # trot10 @ ibm 20: legs 0, 3 in swing
    ss = torch.zeros((B, 4), device=DEV)
    stance = torch.ones((B, 4), device=DEV); stance[:, 0] = 0; stance[:, 3] = 0
    f_plan = lambda: eng.plan(0, plan, x0, vb, yr, root_states=rs)
    f_st = lambda: eng.stance_torques(jac, stance, u0, tau)
    f_leg = lambda: eng.leg_torques(tick, 20, vb, yr, gait, th, pf, fpb, fvb, jac, u0, mem, tau, root_states=rs)
    pt, vt = torch.zeros((B, 4, 3), device=DEV), torch.zeros((B, 4, 3), device=DEV)
    f_leg_all = lambda: eng.leg_torques(tick, 20, vb, yr, gait, th, pf, fpb, fvb, jac, u0, mem, tau, root_states=rs,
                                        swing_state=ss, pos_target=pt, vel_target=vt)
    # alternate the three so drift hits them alike
    r = {"plan": [], "stance_torques": [], "leg_torques": [], "leg_torques_all_outputs": []}
    for _ in range(2):
        r["plan"] += timeit(f_plan, reps=3)
        r["stance_torques"] += timeit(f_st, reps=3)
        r["leg_torques"] += timeit(f_leg, reps=3)
        r["leg_torques_all_outputs"] += timeit(f_leg_all, reps=3)
    f_leg(); torch.cuda.synchronize()
    res[B] = {k: dict(median_us=float(np.median(v)), min_us=float(min(v)), max_us=float(max(v))) for k, v in r.items()}
    res[B]["swing_fraction"] = float((mem.view(B, 4, 8)[:, :, 1] != 0).float().mean().item())
    # graph replay: device time of the launches without the host's enqueue cost
    for name, fn in (("plan", f_plan), ("stance_torques", f_st), ("leg_torques", f_leg)):
        s = torch.cuda.Stream(device=DEV); s.wait_stream(torch.cuda.current_stream(DEV))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(100):
                if name == "plan": eng.plan(0, plan, x0, vb, yr, root_states=rs, stream=s)
                elif name == "stance_torques": eng.stance_torques(jac, stance, u0, tau, stream=s)
                else: eng.leg_torques(tick, 20, vb, yr, gait, th, pf, fpb, fvb, jac, u0, mem, tau, root_states=rs, stream=s)
        v = timeit(g.replay, n=30, warm=5, reps=5)
        res[B][name]["graph_us_per_launch"] = float(np.median(v)) / 100
print(json.dumps(res, indent=1))

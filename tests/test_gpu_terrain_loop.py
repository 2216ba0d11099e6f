"""GPU: the terrain stage inside the loop on the device -- BatchedController.step_fused ->
BatchedPlant.step -> BatchedTerrain.update with nothing on the host, one robot per scenario of
terrain_ref.LOOP_SCENARIOS in one fleet on per-robot planes (level; 0.1 rad uphill, across,
downhill; 0.2 rad uphill; two dropped starts), 800 ticks, held to the CPU oracle loop's recorded
figures (tests/golden/terrain_loop.npz, asserted by tests/test_terrain_loop.py) by the rule of
tests/test_gpu_plant.py for plant_ref.CLOSED_LOOP: each robot's worst height error and roll /
pitch within twice the recorded value (a floor of 1e-6 rad where the recorded one is rounding
noise), its mean speed within 0.05 m/s.  The two loops drift apart sample by sample at contact
events; the gait-averaged quantities do not.

Asserted on the device's own run as on the CPU loop (terrain_ref.loop_figures, on the swing
memory of the controller and the records of the stage): every swing leg's foothold within 1e-6 m
of the plant's plane, measured vertically, on every clean tick and on the last tick of every
swing; the fitted normal as stored within F32_BOUND = 2.4e-7 of the plane's float32 normal;
every fit accepted after the seed tick; every status 0.  ground="surface" on level ground puts
the footholds at 2 touchdown_z, the fitted plane handed over as it is.

Measured on the MI355X: see DESIGN.md 4.4g (the tests print the figures).
"""
import os

import numpy as np
import pytest

# torch first: it brings its own HIP runtime, which must be loaded before libmpcqp.so
torch = pytest.importorskip("torch")

import plant_ref as pr  # noqa: E402
import terrain_ref as tr  # noqa: E402
from helpers import DEV, _dev  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "terrain_loop.npz")
FOOTHOLD_BOUND = 1e-6
F32_BOUND = 2.4e-7


def device_loop(scenarios, ticks, ground=None):
    """The scenarios in one fleet: returns the run in the layout of plant_ref.closed_loop (what
    terrain_ref.loop_figures reads) and whether any status was not OK."""
    from mpcqp import BatchedTerrain
    from mpcqp.controller import BatchedController
    from mpcqp.plant import BatchedPlant
    B = len(scenarios)
    planes = tr.loop_planes(scenarios)
    par = pr.Params()
    ctl = BatchedController(B, horizon=tr.LOOP["horizon"], robot=tr.LOOP["robot"], gait="TROTTING10",
                            iterations_between_mpc=tr.LOOP["ibm"])
    plant = BatchedPlant(B, controller=ctl, plane=planes, foot_mass=par.foot_mass, substeps=par.substeps,
                         ground_z=par.ground_z, contact_tol=par.contact_tol)
    ter = BatchedTerrain(B, controller=ctl) if ground is None else BatchedTerrain(B, controller=ctl, ground=ground)
    geom = plant.geometry.cpu().numpy()
    root0, dofs0 = pr.stand_pose(B, geom, par, height=tr.loop_heights(scenarios))
    pl = planes.astype(np.float64)
    root0, _ = pr.tilt_pose(root0, np.arctan2(np.hypot(pl[:, 0], pl[:, 1]), pl[:, 2]), np.arctan2(-pl[:, 1], -pl[:, 0]), par)
    root, dofs = plant.reset(root_states=root0, dof_states=dofs0)
    vb = torch.zeros((B, 3), dtype=torch.float64, device=DEV)
    vb[:, 0] = torch.as_tensor([s[3] for s in scenarios], dtype=torch.float64)
    ctl.set_command(vb, 0.0)
    f64 = dict(dtype=torch.float64, device=DEV)
    body = torch.zeros((ticks, B, 13), **f64)
    rec = torch.zeros((ticks, B, 5), **f64)
    foothold = torch.zeros((ticks, B, 4, 3), **f64)
    swing = torch.zeros((ticks, B, 4), dtype=torch.float32, device=DEV)
    touch = torch.zeros((ticks, B, 4), dtype=torch.float32, device=DEV)
    bad = torch.zeros((B,), dtype=torch.int32, device=DEV)
    for it in range(ticks):
        ctl.step_fused(it, None, None, root, dofs, outputs=True)
        plant.step(ctl.tau)
        ter.update()
        body[it] = plant.state[:, :13]
        rec[it] = ter.terrain_state[:, 13:18]
        foothold[it] = ctl.swing_mem.view(B, 4, 8)[:, :, 5:8]
        swing[it] = ctl.swing_state
        touch[it] = plant.touch
        bad |= ctl.status | plant.status | ter.status
    torch.cuda.synchronize()
    body = body.cpu().numpy()
    roll, pitch = zip(*(pr.euler_zyx(h[:, 3:7]) for h in body))
    rec = rec.cpu().numpy()
    run = dict(height=body[:, :, 2], x=body[:, :, 0], roll=np.stack(roll), pitch=np.stack(pitch), dt=par.dt_control,
               swing=swing.cpu().numpy() > 0, touch=touch.cpu().numpy(), foothold=foothold.cpu().numpy(),
               plane=rec[:, :, :4], fitted=rec[:, :, 4] != 0.0, planes=planes)
    return run, bad.cpu().numpy(), ter, ctl


def test_the_loop_with_the_terrain_stage_on_the_device():
    fx = dict(np.load(GOLDEN))
    names = [s[0] for s in tr.LOOP_SCENARIOS]
    assert fx["names"].tolist() == names and int(fx["ticks"]) == tr.LOOP_TICKS
    run, bad, ter, ctl = device_loop(tr.LOOP_SCENARIOS, tr.LOOP_TICKS)
    assert (bad == 0).all() and np.isfinite(run["height"]).all() and np.isfinite(run["plane"]).all()
    assert run["fitted"][1:].all() and bool(ter.fitted.all()) and ter.ground == "feet"
    fig = tr.loop_figures(run)
    print()
    for b, name in enumerate(names):
        print(f"  {name:34s} height {fig['height'][b]:.5f} ({fx['height'][b]:.5f})  roll / pitch {fig['tilt'][b]:.3g} "
              f"({fx['tilt'][b]:.3g})  speed {fig['speed'][b]:.4f} ({fx['speed'][b]:.4f})  foothold {fig['foothold'][b]:.1e} "
              f"touchdown {fig['touchdown'][b]:.1e} any {fig['foothold_any'][b]:.1e}  normal {fig['normal'][b]:.1e} "
              f"clean {fig['clean'][b]:.3f} from {fig['start'][b]}")
    assert (fig["height"] <= 2 * fx["height"]).all()
    assert (fig["tilt"] <= np.maximum(2 * fx["tilt"], 1e-6)).all()
    assert (np.abs(fig["speed"] - fx["speed"]) <= 0.05).all()
    assert (fig["foothold"] <= FOOTHOLD_BOUND).all() and (fig["touchdown"] <= FOOTHOLD_BOUND).all()
    assert (fig["normal"] <= F32_BOUND).all()
    assert (fig["clean"] >= 0.97).all() and (fig["start"] <= 110).all()
    # the cone rows read the fitted normal, the swing leg the plane of the stage
    assert torch.equal(ctl.robot[:, 9:12], ter.normal) and torch.equal(ter.plane[:, :3], ter.normal)
    d = ter.terrain_state[:, 16] - ter.terrain_state[:, 15] * ctl.engine.touchdown_z
    assert torch.equal(ter.plane[:, 3], d.to(torch.float32))


def test_surface_convention_on_level_ground():
    """ground="surface": the fitted (n, d) is the swing leg's ground as it is, and on the plant's
    level ground, where the foot centres ride at ground_z = touchdown_z, every foothold lies at
    2 touchdown_z."""
    sc = tr.LOOP_SCENARIOS[:2]
    run, bad, ter, ctl = device_loop(sc, 300, ground="surface")
    assert (bad == 0).all() and run["fitted"][1:].all() and ter.ground == "surface"
    fig = tr.loop_figures(run, last=100)
    z = run["foothold"][..., 2][run["swing"] & (np.arange(300) > 1)[:, None, None]]
    print(f"\nsurface convention: foothold z {z.min():.6f} .. {z.max():.6f}, off the plane by {fig['foothold']}")
    assert np.abs(z - 2 * tr.TOUCHDOWN_Z).max() <= FOOTHOLD_BOUND
    assert np.abs(fig["foothold"] - 0.0255).max() <= FOOTHOLD_BOUND
    assert torch.equal(ter.plane[:, 3], ter.terrain_state[:, 16].to(torch.float32))

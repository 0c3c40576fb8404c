"""Film a world with two flies: the two flies of ``actuators_and_two_flies.py`` through a fixed camera above them and one
tracking camera each, saved as GIFs.  Run from the repo root:  python examples/render_two_flies.py [out_dir]

A world with several flies is stepped as one batch per fly; ``set_renderer(..., flies="all")`` composes the flies' batches in
one image (the nearest surface wins).  Each tracking camera follows its own fly.
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch

from flygym_amd import HIPSimulation
from flygym_amd.anatomy import ActuatedDOFPreset, AxisOrder, JointPreset, Skeleton
from flygym_amd.compose import ActuatorType, FlatGroundWorld, Fly, KinematicPosePreset
from flygym_amd.utils.math import Rotation3D

out = Path(sys.argv[1]) if len(sys.argv) > 1 else Path("render_two_flies")
n = 16


def make_fly(name, preset):
    fly = Fly(name=name)
    fly.add_joints(Skeleton(axis_order=AxisOrder.YAW_PITCH_ROLL, joint_preset=preset), neutral_pose=KinematicPosePreset.NEUTRAL)
    return fly, fly.skeleton.get_actuated_dofs_from_preset(ActuatedDOFPreset.LEGS_ACTIVE_ONLY)


# alice: position servos + controllable dampers; bob: muscles on the knees, integrated-velocity servos elsewhere
alice, dofs = make_fly("alice", JointPreset.LEGS_ONLY)
alice.add_actuators(dofs, ActuatorType.POSITION, kp=50.0, neutral_input=KinematicPosePreset.NEUTRAL)
alice.add_actuators(dofs, ActuatorType.DAMPER, kv=2e-3, ctrlrange=(0.0, 5.0))
alice.add_leg_adhesion()
bob, dofs_b = make_fly("bob", JointPreset.LEGS_ACTIVE_ONLY)
knees = [d for d in dofs_b if "tibia" in d.name]
rest = [d for d in dofs_b if d not in knees]
bob.add_actuators(knees, ActuatorType.MUSCLE, lengthrange=(-3.0, 1.0), force=3.0, timeconst=(0.003, 0.01), forcerange=(-30.0, 30.0))
bob.add_actuators(rest, ActuatorType.INTVELOCITY, kp=40.0, kv=1e-3, actrange=(-2.5, 2.5))
cam_a, cam_b = alice.add_tracking_camera(), bob.add_tracking_camera()
above = dict(name="above", mode="fixed", pos=(5.0, 0.0, 18.0), rotation=Rotation3D("xyaxes", (1, 0, 0, 0, 1, 0)), fovy=45.0)

world = FlatGroundWorld()
world.add_fly(alice, (0, 0, 0.8), Rotation3D("quat", (1, 0, 0, 0)))
world.add_fly(bob, (8.0, 0, 0.9), Rotation3D("quat", (0.9238795, 0, 0, 0.3826834)), add_ground_contact_sensors=False)

sim = HIPSimulation(world, n_worlds=n)
sim.set_leg_adhesion_states("alice", np.ones((n, 6), dtype=np.float32))
sim.warmup(0.02)
# alice brown, bob blue-grey
k = {name: len(fly.get_bodysegs_order()) for name, fly in world.fly_lookup.items()}
renderer = sim.set_renderer([above, cam_a, cam_b], worlds=[0, 5], flies="all", use_gpu_batch_rendering=True,
                            capsule_rgb={"bob": np.tile((0.35, 0.45, 0.6), (k["bob"], 1))})

g = torch.Generator(device=sim.device); g.manual_seed(0)
for tick in range(100):                            # 0.2 s in 20-step launches: a frame every 8 ms
    sim.set_actuator_inputs("alice", ActuatorType.DAMPER, torch.full((n, len(dofs)), float(tick % 5), device=sim.device))
    sim.set_actuator_inputs("bob", ActuatorType.MUSCLE, torch.rand((n, len(knees)), device=sim.device, generator=g))
    sim.set_actuator_inputs("bob", ActuatorType.INTVELOCITY, 4.0 * (torch.rand((n, len(rest)), device=sim.device, generator=g) - 0.5))
    sim.step(20)
    sim.render_as_needed()
print(f"{len(renderer.frames)} frames of {tuple(renderer.frames[0].shape)} (worlds, cameras, H, W, 3) on {renderer.frames[0].device}; "
      f"cameras {renderer.enabled_cam_names}")
renderer.save_video(0, out)                        # several cameras: a directory with one GIF per camera
for f in sorted(out.glob("*.gif")):
    print(f"saved {f} ({f.stat().st_size / 1024:.0f} KiB)")

"""Look at the flies you simulate: 256 flies walk over the blocks terrain with a tripod gait, four of them are filmed by the
tracking camera, and the film is saved as a GIF.  Run from the repo root:  python examples/render_a_walk.py [out.gif]

The loop is the reference's own (``sim.set_renderer(cam, worlds=[...], use_gpu_batch_rendering=True)`` once,
``sim.render_as_needed()`` after each step or launch, ``renderer.save_video(...)`` at the end); frames stay on the GPU
until they are saved.
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np

from flygym_amd import HIPSimulation, make_model
from flygym_amd.compose import BlocksTerrainWorld
from flygym_amd.controllers import TripodCPG
from flygym_amd.utils.math import Rotation3D

out = Path(sys.argv[1]) if len(sys.argv) > 1 else Path("render_a_walk.gif")
n = 256
fly, _, cam = make_model()                         # the fly of the benchmark with its tracking camera
world = BlocksTerrainWorld()
world.add_fly(fly, (0, 0, 0.8), Rotation3D("quat", (1, 0, 0, 0)))
sim = HIPSimulation(world, n_worlds=n)
sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
sim.warmup()

renderer = sim.set_renderer(cam, worlds=[0, 85, 170, 255], use_gpu_batch_rendering=True)   # 240 x 320, a frame every 8 ms
table = TripodCPG(fly.get_actuated_jointdofs_order("position"), sim.timestep).targets(n, 2500, device=sim.device)
ids = sim.replay_ids(fly.name)
for tick in range(125):                            # 0.25 s of walking in 20-step launches
    sim.step_replay(table, ids, 20 * tick, 20)
    sim.render_as_needed()
x = sim.get_body_positions(fly.name)[:, 0, 0]
print(f"walked {x.mean().item():.2f} mm on average; {len(renderer.frames)} frames of {tuple(renderer.frames[0].shape)} on {renderer.frames[0].device}")
renderer.save_video([0, 85, 170, 255], out, scale=0.5)      # the four worlds in a 2 x 2 grid; a single world id saves that world alone
print(f"saved {out} ({out.stat().st_size / 1024:.0f} KiB)")

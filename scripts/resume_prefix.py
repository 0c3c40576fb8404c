"""Contact-space solve: how much of a step's later eliminations repeats the one before (diagnostic build, on the GPU).

dual_eliminate takes its pivots in ascending row order, so an elimination whose pivot set agrees with the previous one's on every
row below the first differing row recomputes that many leading pivots bit for bit.  This counts, on bench.py's headline workload
(4096 LEGS_ONLY flies, flat ground, tripod CPG, 50 steps per launch, the bench's settle and warm-up), every elimination beyond a
step's first by (its pivot count n, shared leading pivots k), and prices what resuming at ordinal k would save with the
elimination's measured cost of 52 + 2 p vector instructions at pivot ordinal p.

    python scripts/resume_prefix.py [--build] [--worlds=4096] [--steps=1000] [--terrain=blocks] > profiles/resume_prefix.txt
"""
import ctypes, math, subprocess, sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import numpy as np, torch
from flygym_amd import _native
lib_prof = ROOT / "build" / "libnmf_prof.so"      # (the stage-profile build: never beside the product library)
lib_prof.parent.mkdir(exist_ok=True)
if "--build" in sys.argv or not lib_prof.exists():
    subprocess.run(_native.compile_command(lib_prof, ["-DNMF_STAGE_PROFILE"]), check=True)
    if "--build" in sys.argv: sys.exit(0)
_native.LIB_PATH = lib_prof
from flygym_amd import HIPSimulation, make_model
from flygym_amd.compose import ActuatorType
from flygym_amd.controllers import TripodCPG

opt = lambda name, default: next((a.split("=")[1] for a in sys.argv if a.startswith(f"--{name}=")), default)
n, steps, terrain = int(opt("worlds", 4096)), int(opt("steps", 1000)), opt("terrain", "flat")
STEP_VALU = 5728.0      # vector instructions per env-step of the headline kernel before the change (SQ_INSTS_VALU, profiles/resume_summary.md; round 6: 6071)
fly, world, _ = make_model()
if terrain != "flat":
    import flygym_amd.compose as C
    from flygym_amd.utils.math import Rotation3D
    world = {"gapped": C.GappedTerrainWorld, "blocks": C.BlocksTerrainWorld, "mixed": C.MixedTerrainWorld}[terrain]()
    world.add_fly(fly, (0, 0, 0.8), Rotation3D("quat", (1, 0, 0, 0)))
sim = HIPSimulation(world, n_worlds=n, device=0)
L = _native.lib()
L.nmf_debug_resume_hist.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
table = TripodCPG(fly.get_actuated_jointdofs_order(ActuatorType.POSITION), sim.timestep).targets(n, 2500, device=sim.device)
ids = sim.replay_ids(fly.name)
sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
sim.step(500)                                       # bench.py's settle: neutral, one gait cycle, then its default --warmup
cursor = 0
for _ in range((int(math.ceil(1.0 / (12.0 * sim.timestep) / 50.0)) * 50 + 500) // 50):
    sim.step_replay(table, ids, cursor, 50); cursor += 50
n_hist = L.nmf_debug_resume_hist(None, 0, 0)          # the library says how large its histogram is: rows x 65
assert n_hist > 0 and n_hist % 65 == 0
ROWS = n_hist // 65
buf = (ctypes.c_ulonglong * n_hist)()
assert L.nmf_debug_resume_hist(buf, n_hist, 1) == 0
sums0 = sim.field("stats_sum").clone()
for _ in range(steps // 50):
    sim.step_replay(table, ids, cursor, 50); cursor += 50
assert L.nmf_debug_resume_hist(buf, n_hist, 0) == 0
dsum = (sim.field("stats_sum") - sums0).double().sum(dim=0).cpu().numpy()
H = np.array(list(buf), dtype=np.float64).reshape(ROWS, 65)
solves, later = H[ROWS - 1, 0], H[:65]
env_steps = float(n * steps)
per_m = 1e6 / env_steps
cost = lambda p: 52.0 * p + p * (p - 1.0)          # sum of 52 + 2 q over q < p
N, K = np.meshgrid(np.arange(65), np.arange(65), indexing="ij")
print(f"{n} worlds x {steps} steps, {terrain} ground: {env_steps:.0f} env-steps; contacts {dsum[1] / dsum[0]:.2f}, eliminations {dsum[2] / dsum[0]:.3f} per step (stats_sum)")
print(f"per million env-steps: contact-space solves {solves * per_m:.0f}, eliminations beyond a step's first {later.sum() * per_m:.0f} "
      f"({later.sum() / env_steps:.3f} per step)")
print(f"later eliminations: mean pivots n {(later * N).sum() / later.sum():.2f}, mean shared prefix k {(later * K).sum() / later.sum():.2f}, "
      f"mean k / n {(later * K / np.maximum(N, 1)).sum() / later.sum():.3f}, identical set (k = n) {later[N == K].sum() / later.sum():.3f}")
print("\nshared prefix k: later eliminations per million env-steps, share, cumulative share")
byk = later.sum(axis=0)
for k in range(65):
    if byk[k]: print(f"  k {k:2d}  {byk[k] * per_m:10.0f}  {byk[k] / later.sum():6.3f}  {byk[:k + 1].sum() / later.sum():6.3f}")
print("\npivot count n of those eliminations: per million env-steps, share, mean k at that n")
byn = later.sum(axis=1)
for i in range(65):
    if byn[i]: print(f"  n {i:2d}  {byn[i] * per_m:10.0f}  {byn[i] / later.sum():6.3f}  {(later[i] * np.arange(65)).sum() / byn[i]:6.2f}")
print(f"\nvector instructions (52 + 2 p at ordinal p) per env-step, against the step's {STEP_VALU:.0f}:")
print(f"  all later eliminations                      {(later * cost(N)).sum() / env_steps:8.1f}  {100 * (later * cost(N)).sum() / env_steps / STEP_VALU:5.2f} %")
for stride, cap in ((1, 64), (2, 64), (4, 64), (1, 16), (4, 16), (8, 16), (1, 8), (4, 8), (8, 8)):
    Kr = np.minimum(K // stride * stride, cap)
    saved = (later * cost(Kr)).sum() / env_steps
    print(f"  saved resuming at min(k rounded down to {stride}, {cap:2d}) {saved:8.1f}  {100 * saved / STEP_VALU:5.2f} %")

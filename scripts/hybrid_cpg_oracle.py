"""The hybrid controller's rules on the float64 CPU oracle, one world (no GPU): (a) the distribution of the quantities the rules
threshold — the swing legs' sensor force along the body's x axis and the depth of the deepest leg below the third deepest — over
open-loop walking at the unit drive, 500-step settle + 10 000 steps, on flat and on gapped ground, with the rate at which each rule
would fire at the given thresholds; (b) distance travelled over 10 000 steps, hybrid against CPG only, in 20-step ticks, on the
gapped, blocks and mixed terrains.  Prints the lines profiles/hybrid_cpg.txt records.
usage: python scripts/hybrid_cpg_oracle.py [stats|walk] [retraction_threshold] [stumbling_force_threshold]"""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "tests", ROOT / "oracle"):
    sys.path.insert(0, str(p))
import numpy as np
import cpg_spec, hybrid_spec as spec, oracle as orc
import flygym_amd.compose as C
from flygym_amd import make_model
from flygym_amd.anatomy import LEGS
from flygym_amd.controllers import STUMBLING_DEFAULT, HybridTurningCPG, TripodCPG
from flygym_amd.utils.math import Rotation3D

what = sys.argv[1] if len(sys.argv) > 1 else "stats"
thr_h = float(sys.argv[2]) if len(sys.argv) > 2 else 0.05
thr_f = float(sys.argv[3]) if len(sys.argv) > 3 else STUMBLING_DEFAULT
DT, STEPS, TICK = 1e-4, 10000, 20
WORLDS = {"flat": C.FlatGroundWorld, "gapped": C.GappedTerrainWorld, "blocks": C.BlocksTerrainWorld, "mixed": C.MixedTerrainWorld}
orc.build()


def setup(kind):
    fly = make_model()[0]
    world = WORLDS[kind]()
    world.add_fly(fly, (0, 0, 0.8), Rotation3D("quat", (1, 0, 0, 0)))
    model = world.compile_model()
    cpg = TripodCPG(fly.get_actuated_jointdofs_order("position"), DT)
    segs = [s.name for s in fly.get_bodysegs_order()]
    info = dict(swing=~cpg.stance_bins(model, fly), root=segs.index(fly.root_segment.name),
                tips=np.array([segs.index(f"{leg}_tarsus5") for leg in LEGS]), corr=HybridTurningCPG.correction_row(cpg.actuated_dofs),
                contact=bool(model["sem_options"][2]))
    o = orc.Oracle(model.to_blob(), "f64")
    o.ctrl[42:] = 1.0
    o.step(500)
    return cpg, info, o


def views(o):
    return [np.array(o.arr(k))[None] for k in ("seg_xpos", "seg_xquat", "sensordata")]


def stats(kind):
    cpg, info, o = setup(kind)
    rows, phases, _, _, _ = cpg_spec.rollout(cpg.cycle, cpg.leg_of_dof, cpg_spec.reset_phases(1), np.ones((1, 6)), np.ones((1, 2)), STEPS, timestep=DT)
    table, ids = np.ascontiguousarray(rows[0], dtype=np.float32), np.arange(42, dtype=np.int32)
    push, excess, fired = [], [], np.zeros(2, dtype=int)
    for s in range(STEPS):
        xpos, xquat, sd = views(o)
        h = spec.heights(xpos, info["root"], info["tips"])[0]
        excess.append(np.sort(h)[-1] - np.sort(h)[-3])
        found, F = spec.world_forces(sd, info["contact"])
        p = (F[0] * spec.x_axis(xquat.reshape(1, -1, 4)[:, info["root"]])[0]).sum(axis=1)
        sw = info["swing"][spec.start_bins(phases[:, s], cpg.n_bins)[0], np.arange(6)] & (found[0] > 0)
        push.extend(p[sw].tolist())
        flags = spec.decide(xpos, xquat, sd, phases[:, s], info["swing"], info["root"], info["tips"], retraction_threshold=thr_h,
                            stumbling_force_threshold=thr_f, contact_frame=info["contact"])[0]
        fired += [int((flags & 1).any()), int((flags & 2).any())]
        o.step_replay(table, ids, s, 1)
    push, excess = np.array(push), np.array(excess)
    q = lambda a, qs: ", ".join(f"{v:.4g}" for v in np.quantile(a, qs))
    print(f"{kind}: open-loop unit drive, {STEPS} steps, x travelled {o.qpos[0]:.2f} mm")
    print(f"  F . xhat of swinging legs in contact ({len(push)} leg-steps): min {push.min():.4g}, quantiles 0.001 / 0.01 / 0.1 / 0.5 / 0.9: {q(push, [0.001, 0.01, 0.1, 0.5, 0.9])}, max {push.max():.4g}")
    print(f"  h of the deepest leg - third largest h: quantiles 0.5 / 0.9 / 0.99 / 0.999: {q(excess, [0.5, 0.9, 0.99, 0.999])}, max {excess.max():.4g} mm")
    print(f"  at thresholds ({thr_h} mm, {thr_f}): steps with a retraction {fired[0]} ({fired[0] / STEPS:.2%}), with a stumble {fired[1]} ({fired[1] / STEPS:.2%})")


def walk(kind, hybrid):
    cpg, info, o = setup(kind)
    th, r = cpg_spec.reset_phases(1), np.ones((1, 6))
    rho, sigma = np.zeros((1, 6)), np.zeros((1, 6))
    x0, ids, fired = float(o.qpos[0]), np.arange(42, dtype=np.int32), np.zeros(2, dtype=int)
    for _ in range(STEPS // TICK):
        flags = np.zeros((1, 6), dtype=np.uint8)
        if hybrid:
            flags = spec.decide(*views(o), th, info["swing"], info["root"], info["tips"], retraction_threshold=thr_h,
                                stumbling_force_threshold=thr_f, contact_frame=info["contact"])
        fired += [int((flags & 1).any()), int((flags & 2).any())]
        rows, _, _, _, th, r, rho, sigma = spec.rollout(cpg.cycle, cpg.leg_of_dof, th, r, np.ones((1, 2)), TICK, timestep=DT, flags=flags,
                                                        retraction=rho, stumbling=sigma, corr=info["corr"])
        o.step_replay(np.ascontiguousarray(rows[0], dtype=np.float32), ids, 0, TICK)
    ok = bool(np.isfinite(o.qpos).all())
    print(f"{kind}, {'hybrid' if hybrid else 'CPG only'}: x travelled {float(o.qpos[0]) - x0:+.2f} mm, y {float(o.qpos[1]):+.2f} mm, finite {ok}; "
          f"ticks with a retraction {fired[0]}, with a stumble {fired[1]} of {STEPS // TICK}", flush=True)


if what == "stats":
    for kind in ("flat", "gapped"):
        stats(kind)
else:
    print(f"float64 oracle, one world, {STEPS} steps in {TICK}-step ticks, thresholds ({thr_h} mm, {thr_f})")
    for kind in ("gapped", "blocks", "mixed"):
        for hybrid in (False, True):
            walk(kind, hybrid)

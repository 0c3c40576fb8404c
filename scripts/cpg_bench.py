"""Closed-loop CPG timing (needs the GPU): ``TurningCPG.advance(20)`` at 4096 worlds and 48 columns (42 position targets + 6
adhesion), HIP events around 200 launches after 20 warm-up launches, against (a) the torch table builder producing the same 20
rows — ``TripodCPG.targets(4096, 20, start_step=k, device=..., adhesion=...)``, the only way before the controller existed — and
(b) the launch's write-traffic floor, 4096 x 20 x 48 x 4 B at the achievable HBM bandwidth.  Writes profiles/turning_cpg.txt (or
the path given).  ``--hybrid`` adds a line: ``HybridTurningCPG.advance(20)`` on the same batch in the same session, and its ratio;
the lines are then appended, under a heading, to profiles/hybrid_cpg.txt (or the path given) and turning_cpg.txt is left alone."""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import numpy as np, torch
from flygym_amd import HIPSimulation, make_model
from flygym_amd.controllers import HybridTurningCPG, TurningCPG

HYBRID = "--hybrid" in sys.argv
paths = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = Path(paths[0]) if paths else ROOT / "profiles" / ("hybrid_cpg.txt" if HYBRID else "turning_cpg.txt")
N, STEPS, WARMUP, REPS = 4096, 20, 20, 200
HBM_ACHIEVABLE = 5.0e12            # B/s: what a streaming kernel reaches on an MI355X (8 TB/s peak)
PHYSICS_MS = 1.35                  # 20-step physics launch at 4096 worlds (BENCH_r06.json)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(reps):
        fn(k)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


fly, world, _ = make_model()
sim = HIPSimulation(world, n_worlds=N, device=0)
cpg = TurningCPG(sim, fly.name, adhesion=(20.0, 1.0))
rng = np.random.default_rng(0)
cpg.set_drive(rng.uniform(0.4, 1.2, (N, 2)).astype(np.float32))
adhesion = (cpg.stance, 20.0, 1.0)
lines = [f"TurningCPG.advance({STEPS}), {N} worlds, {cpg.n_act} columns, table_steps {cpg.table_steps}; device events around {REPS} "
         f"launches after {WARMUP} warm-up launches, three windows each"]
timed(lambda k: cpg.advance(STEPS), WARMUP)
kernel = [timed(lambda k: cpg.advance(STEPS), REPS) for _ in range(3)]
timed(lambda k: cpg.targets(N, STEPS, start_step=STEPS * k, device=sim.device, adhesion=adhesion), WARMUP)
builder = [timed(lambda k: cpg.targets(N, STEPS, start_step=STEPS * k, device=sim.device, adhesion=adhesion), REPS) for _ in range(3)]
one = [timed(lambda k: cpg.advance(1), REPS) for _ in range(3)]
full = [timed(lambda k: cpg.advance(cpg.table_steps), REPS) for _ in range(3)]
best, tb = min(kernel), min(builder)
bytes_written = N * STEPS * cpg.n_act * 4
floor_ms = bytes_written / HBM_ACHIEVABLE * 1e3
lines.append(f"nmf_cpg_advance_kernel: {best * 1e3:.1f} us per launch (windows {', '.join(f'{v * 1e3:.1f}' for v in kernel)})")
lines.append(f"torch table builder, the same {STEPS} rows: {tb * 1e3:.1f} us per call (windows {', '.join(f'{v * 1e3:.1f}' for v in builder)}) "
             f"= {tb / best:.1f} x the kernel")
lines.append(f"write-traffic floor: {bytes_written / 1e6:.1f} MB at {HBM_ACHIEVABLE / 1e12:.1f} TB/s = {floor_ms * 1e3:.1f} us; the launch is at "
             f"{floor_ms / best:.2f} of it ({bytes_written / (best * 1e-3) / 1e12:.2f} TB/s of rows)")
lines.append(f"advance(1): {min(one) * 1e3:.1f} us, advance({cpg.table_steps}): {min(full) * 1e3:.1f} us per launch: "
             f"{(min(full) - min(one)) / (cpg.table_steps - 1) * 1e3:.2f} us per further step (the recurrence is a dependent chain per step, "
             f"the rows stream)")
lines.append(f"share of the {STEPS}-step physics launch ({PHYSICS_MS} ms, BENCH_r06.json): {best / PHYSICS_MS * 100:.1f} %")
if HYBRID:
    sim.step(500)                                  # settled flies: real pose and sensor values for the rules to read
    with HybridTurningCPG(sim, fly.name, adhesion=(20.0, 1.0)) as hyb:
        hyb.set_drive(cpg.drive)
        timed(lambda k: hyb.advance(STEPS), WARMUP)
        pairs = [(timed(lambda k: hyb.advance(STEPS), REPS), timed(lambda k: cpg.advance(STEPS), REPS)) for _ in range(3)]
        hb, pb = min(p[0] for p in pairs), min(p[1] for p in pairs)
        lines.append(f"nmf_cpg_advance_hybrid_kernel: {hb * 1e3:.1f} us per launch (windows {', '.join(f'{p[0] * 1e3:.1f}' for p in pairs)}), "
                     f"interleaved with advance({STEPS}) at {pb * 1e3:.1f} us (windows {', '.join(f'{p[1] * 1e3:.1f}' for p in pairs)}): "
                     f"ratio {hb / pb:.3f}; flags set in the last launch: {int(hyb.rule_flags.count_nonzero())} of {N * 6}")
assert best < tb, "the kernel must be faster than the torch builder"
cpg.close()
out_path.parent.mkdir(parents=True, exist_ok=True)
if HYBRID:
    with open(out_path, "a") as f:
        f.write("\n== MI355X: scripts/cpg_bench.py --hybrid ==\n" + "\n".join(lines) + "\n")
else:
    out_path.write_text("\n".join(lines) + "\n")
print("\n".join(lines))

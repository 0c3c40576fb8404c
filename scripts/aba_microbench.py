"""Cycles per articulated-body sweep, in isolation (diagnostic).  usage: aba_microbench.py [--build] [--pair]

--pair: the two solves of an ordinary step (smooth, then Euler's on the same configuration) timed together, both ways: Euler on
the factors the smooth sweep stored (the shipped build), the same with the sweep's rank-1 downdates on the vector pipe
(-DNMF_ABA_RANK1_VALU), and Euler factorising for itself (-DNMF_EULER_REFACTOR)."""
import ctypes, subprocess, sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from flygym_amd import _native
pair = "--pair" in sys.argv
variants = {"stored": [], "rank1_valu": ["-DNMF_ABA_RANK1_VALU"], "refactor": ["-DNMF_EULER_REFACTOR"]} if pair else {"": []}
libs = {k: ROOT / "flygym_amd" / f"libnmf_hip_aba{'_' + k if k else ''}.so" for k in variants}
if "--build" in sys.argv or not all(p.exists() for p in libs.values()):
    procs = [subprocess.Popen(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-mllvm", "-amdgpu-sched-strategy=iterative-ilp",
                               *_native.MATH_FLAGS, "-mllvm", "-amdgpu-atomic-optimizer-strategy=None", "-fPIC", "-shared", "-DNMF_TOPO_MASK=1", *variants[k],
                               f"-I{ROOT/'include'}", f"-I{ROOT/'flygym_amd/csrc'}", "-x", "hip", str(ROOT / "scripts/aba_microbench.hip"), "-o", str(libs[k])]) for k in variants]
    if any(p.wait() != 0 for p in procs): sys.exit(1)
    if "--build" in sys.argv: sys.exit(0)
import numpy as np, torch
from flygym_amd import HIPSimulation, make_model
fly, world, _ = make_model()
for key, lib_path in libs.items():
    _native.LIB_PATH, _native._lib = lib_path, None
    for n in (1, 2048):
        sim = HIPSimulation(world, n_worlds=n, device=0)
        sim.set_leg_adhesion_states(fly.name, np.ones((n, 6), dtype=np.float32))
        sim.step(600); torch.cuda.synchronize()
        L = _native.lib()
        L.nmf_aba_bench.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        cyc = torch.zeros(n, dtype=torch.int64, device=sim.device)
        for mode in ((2,) if pair else (0, 1)):
            L.nmf_aba_bench(sim._batch_h, cyc.data_ptr(), 200, mode)
            c = cyc.cpu().numpy()
            what = f"pair (smooth + Euler, {key})" if mode == 2 else f"withK {mode}"
            print(f"n_worlds {n:5d} {what}: cycles  median {np.median(c):.0f}  min {c.min()}  max {c.max()}  (contacts {sim.field('stats')[0,0].item():.0f})")

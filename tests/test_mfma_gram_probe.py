"""The Gram block of the contact-space solve (``flygym_amd/csrc/nmf_dual.h``) builds G = Z Z^T with
``v_mfma_f32_4x4x1_16B_f32`` and relies on two properties of that instruction that the stand-alone probe
``scripts/micro/mfma_gram_probe.hip`` establishes on the GPU:

* a 17-term chain fed one term at a time is bit for bit the chain ``acc = a0 b0; acc = fmaf(a_i, b_i, acc)`` of the vector
  pipe (one rounding per multiply-add; compared as bit patterns with the same chain on the GPU's VALU and with ``fmaf``
  on the host, over inputs whose products need the extra bits, subnormals and signed zeros);
* lane ``4 q + j``, result register ``i`` holds (A of lane ``4 q + i``) x (B of lane ``4 q + j``), checked against a scalar
  triple loop.

Without a GPU: the probe cross-compiles, and the built library's contact-space kernels carry the instruction (one path:
no vector-pipe form of the block is left beside it).
"""

import re
import struct
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
PROBE = ROOT / "scripts" / "micro" / "mfma_gram_probe.hip"
OBJDUMP = Path("/opt/rocm/lib/llvm/bin/llvm-objdump")


def _compile(tmp_path):
    exe = tmp_path / "mfma_gram_probe"
    res = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", str(PROBE), "-o", str(exe)],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    return exe


def _gfx950_code_object(binary: Path, out: Path) -> Path:
    d = binary.read_bytes()
    i = d.find(b"__CLANG_OFFLOAD_BUNDLE__")
    assert i >= 0, f"{binary} holds no offload bundle"
    n = struct.unpack_from("<Q", d, i + 24)[0]
    off = i + 32
    for _ in range(n):
        o, s, tl = struct.unpack_from("<QQQ", d, off)
        off += 24
        triple = d[off:off + tl].decode()
        off += tl
        if "gfx950" in triple:
            out.write_bytes(d[i + o:i + o + s])
            return out
    raise AssertionError(f"{binary} holds no gfx950 code object")


def test_probe_compiles_to_the_matrix_instruction(tmp_path):
    if not OBJDUMP.exists():
        pytest.skip("no llvm-objdump")
    exe = _compile(tmp_path)
    co = _gfx950_code_object(exe, tmp_path / "probe.co")
    asm = subprocess.run([str(OBJDUMP), "-d", "--no-show-raw-insn", str(co)], capture_output=True, text=True).stdout
    assert len(re.findall(r"v_mfma_f32_4x4x1_16b_f32", asm)) >= 17


def test_contact_space_kernels_use_the_matrix_instruction(tmp_path):
    """Every stepping-kernel instantiation with a contact-space solve has the 6 + NDL (root axes + leg hinges) matrix
    instructions of a Gram round; kernels without one (the primal-only ones) have none."""
    if not OBJDUMP.exists():
        pytest.skip("no llvm-objdump")
    from flygym_amd import _native

    _native.build()
    co = _gfx950_code_object(_native.LIB_PATH, tmp_path / "nmf.co")
    asm = subprocess.run([str(OBJDUMP), "-d", "--no-show-raw-insn", "-C", str(co)], capture_output=True, text=True).stdout
    counts = {}
    for blk in re.split(r"\n(?=[0-9a-f]{16} <)", asm):
        head = blk.split("\n", 1)[0]
        if "nmf_step_kernel" in head:
            counts[head[18:]] = len(re.findall(r"v_mfma_f32_4x4x1_16b_f32", blk))
    assert counts, "no stepping kernel in the library"
    headline = [n for k, n in counts.items() if "HybridTopo<0, 0, 6, 3, 2, 1, 1, 1, 1, 1, 1>, false>" in k and "Terrain" not in k]
    assert headline and all(n >= 17 for n in headline), counts
    assert all(n == 0 or n >= 7 for n in counts.values()), counts


@pytest.mark.gpu
def test_mfma_chain_is_the_fmaf_chain_bit_for_bit(tmp_path):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    exe = _compile(tmp_path)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(res.stdout)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "PASS" in res.stdout
    assert " 0 differ" in res.stdout

"""The leg-chain kernels' fused smooth solve (``aba_solve``, ``flygym_amd/csrc/nmf_step_aba.h``) runs the rank-1 downdates of its
articulated inertias on ``v_mfma_f32_4x4x1_16B_f32`` (``grp8_rank1_mfma`` in ``nmf_device.h``).  The stand-alone probe
``scripts/micro/aba_rank1_probe.hip`` includes that header and establishes on the GPU, over 1 048 576 random groups of eight
lanes and chains of 17 successive downdates (subnormals, zeros of both signs, products that need more than 24 bits, ties):

* every lane, shadow lanes included, ends with ``fmaf(nk, U of lane c, IA[c])`` for c = 0 .. 5, word for word what the six
  ``ds_swizzle_b32`` broadcasts + three ``v_pk_fma_f32`` leave, and what ``fmaf`` gives on the host;
* the instruction's own A broadcast (``cbsz:1``, ``abid:0 / 1`` — the form the kernels use) and the form fed by two DPP copies
  (``grp8_lo``: ``row_shr:4 bank_mask:0xa``, ``grp8_hi``: ``row_shl:4 bank_mask:0x5``) agree, and the lane maps of the copies and
  of ``grp8_bcast_dpp`` (the root's D) are the intended ones;
* the pad registers (columns 6 and 7) reach no result: a NaN in the shadow lanes' U and NaN pads carried along the chain change
  nothing.

Without a GPU: the probe cross-compiles to both forms of the instruction.
"""

import re
import struct
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
PROBE = ROOT / "scripts" / "micro" / "aba_rank1_probe.hip"
OBJDUMP = Path("/opt/rocm/lib/llvm/bin/llvm-objdump")


def _compile(tmp_path):
    exe = tmp_path / "aba_rank1_probe"
    res = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT / 'flygym_amd' / 'csrc'}", str(PROBE), "-o", str(exe)],
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


def test_probe_compiles_to_both_forms_of_the_matrix_instruction(tmp_path):
    if not OBJDUMP.exists():
        pytest.skip("no llvm-objdump")
    exe = _compile(tmp_path)
    co = _gfx950_code_object(exe, tmp_path / "probe.co")
    asm = subprocess.run([str(OBJDUMP), "-d", "--no-show-raw-insn", str(co)], capture_output=True, text=True).stdout
    mfma = re.findall(r"v_mfma_f32_4x4x1_16b_f32[^\n]*", asm)
    assert sum("cbsz:1 abid:1" in m for m in mfma) >= 17 and sum("cbsz:1" in m and "abid" not in m for m in mfma) >= 17, len(mfma)
    assert sum("cbsz" not in m for m in mfma) >= 34, len(mfma)                      # the form fed by the DPP copies
    assert len(re.findall(r"row_shr:4 row_mask:0xf bank_mask:0xa", asm)) >= 17 and len(re.findall(r"row_shl:4 row_mask:0xf bank_mask:0x5", asm)) >= 17
    assert len(re.findall(r"ds_swizzle_b32", asm)) >= 6 * 17                          # the form it replaces


@pytest.mark.gpu
def test_mfma_downdate_is_the_swizzle_and_packed_fma_downdate_bit_for_bit(tmp_path):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    exe = _compile(tmp_path)
    res = subprocess.run(["timeout", "-k", "10", "120", str(exe)], capture_output=True, text=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "PASS" in res.stdout
    assert len(re.findall(r": 0 differ", res.stdout)) == 5, res.stdout

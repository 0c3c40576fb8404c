"""LDS / VGPR / spill figures of every stepping-kernel instantiation in the built library (no GPU needed).

--text-sha256: print the SHA-256 of the gfx950 code object's .text section instead (same machine code <=> same digest).
--kernel-sha256: print one SHA-256 per kernel symbol instead: the bytes of that symbol in .text (the kernel descriptors live in
.rodata and are left out), so that a library digest that moved can be traced to the kernels that moved."""
import hashlib
import re
import struct
import subprocess
import sys
import tempfile
from pathlib import Path

paths = [a for a in sys.argv[1:] if not a.startswith("--")]
so = Path(paths[0] if paths else Path(__file__).resolve().parents[1] / "flygym_amd" / "libnmf_hip.so")
d = so.read_bytes()
i = d.find(b"__CLANG_OFFLOAD_BUNDLE__")
n = struct.unpack_from("<Q", d, i + 24)[0]
off = i + 32
with tempfile.TemporaryDirectory() as tmp:
    for _ in range(n):
        o, s, tl = struct.unpack_from("<QQQ", d, off)
        off += 24
        triple = d[off:off + tl].decode()
        off += tl
        if "gfx950" in triple:
            (Path(tmp) / "co.elf").write_bytes(d[i + o:i + o + s])
    if "--text-sha256" in sys.argv:
        subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objcopy", "-O", "binary", "--only-section=.text", f"{tmp}/co.elf", f"{tmp}/text.bin"], check=True)
        print(hashlib.sha256((Path(tmp) / "text.bin").read_bytes()).hexdigest())
        sys.exit(0)
    if "--kernel-sha256" in sys.argv:
        readelf = lambda *a: subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", *a, f"{tmp}/co.elf"], capture_output=True, text=True, check=True).stdout
        # section header line: [Nr] .text PROGBITS <address> <file offset> <size> ...
        nr, addr, foff = re.search(r"\[\s*(\d+)\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)", readelf("-S", "-W")).groups()
        co = (Path(tmp) / "co.elf").read_bytes()
        rows = []
        for line in readelf("--symbols", "-W").splitlines():
            f = line.split()      # Num: Value Size Type Bind Vis Ndx Name
            if len(f) == 8 and f[3] == "FUNC" and f[6] == nr and "kernel" in f[7]:
                start = int(f[1], 16) - int(addr, 16) + int(foff, 16)
                rows.append((subprocess.run(["c++filt", f[7]], capture_output=True, text=True).stdout.strip(), hashlib.sha256(co[start:start + int(f[2])]).hexdigest()))
        for name, digest in sorted(set(rows)):      # (.dynsym and .symtab list a kernel each)
            print(f"{digest}  {name}")
        sys.exit(0)
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", f"{tmp}/co.elf"], capture_output=True, text=True).stdout
for blk in out.split("- .agpr_count")[1:]:
    name = re.search(r"\.name:\s+(\S+)", blk).group(1)
    if "kernel" not in name:
        continue
    g = lambda k: re.search(r"\." + k + r":\s+(\d+)", blk).group(1)
    demangled = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    print(f"{demangled[:110]:110s} lds {g('group_segment_fixed_size'):>6s} vgpr {g('vgpr_count'):>4s} spill {g('vgpr_spill_count'):>3s} scratch {g('private_segment_fixed_size'):>4s}")

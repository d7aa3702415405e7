"""Compare the gfx950 kernels of two builds of libbrush_hip.so, kernel by kernel, without a GPU.

    python tools/kernel_diff.py OLD.so NEW.so
    python tools/kernel_diff.py --resources LIB.so REGEX   # registers / spills / scratch / LDS of matching kernels
    python tools/kernel_diff.py --opcodes OLD.so NEW.so    # also: per-opcode count differences of every CHANGED kernel

For each .so: the device code objects (one per translation unit) are taken out of the .hip_fatbin section and
unbundled with clang-offload-bundler; then, for every kernel symbol of OLD, the llvm-objdump disassembly of the kernel (addresses
and trailing comments stripped: they move when other kernels are added) and the 64 bytes of its kernel descriptor
(<name>.kd) must be identical in NEW.  Kernels only NEW has are listed as new.  Exit status 1 on any difference.
A kernel whose descriptor differs (registers, spills, scratch, LDS) is reported as "CHANGED descriptor", whatever its code.
--opcodes tells a reordering (every count equal), added register moves (only v_mov / s_mov / nop counts differ) and a
different instruction selection (anything else, e.g. one global_load_dwordx3 against three global_load_dword) apart.
--opcodes also gives a third verdict, "REORDERED scalar copies", counted on its own in the summary line and not a
failure: the 64 descriptor bytes are identical, the disassembly lines are the same multiset, and the line sequence is
identical once the s_mov_b32 / s_mov_b64 lines are taken out, i.e. independent scalar register copies changed places
and nothing else did (what moving source text around does to the compositing backward).  Anything else stays CHANGED.
"""
from __future__ import annotations

import collections
import os
import re
import struct
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
LLVM = os.path.join(ROCM, "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def _sections(blob: bytes):
    """{name: (offset, size, addr)} of a 64-bit little-endian ELF."""
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", blob, 0x3A)
    hdrs = [struct.unpack_from("<IIQQQQIIQQ", blob, shoff + i * shentsize) for i in range(shnum)]
    stro = hdrs[shstrndx][4]
    out = {}
    for h in hdrs:
        name = blob[stro + h[0]:blob.index(b"\0", stro + h[0])].decode()
        out[name] = (h[4], h[5], h[3], h)
    return out


def _symbols(blob: bytes, secs):
    """{name: (value, size)} from .symtab."""
    off, size, _, h = secs[".symtab"]
    stroff = secs[".strtab"][0]
    syms = {}
    for i in range(size // 24):
        st_name, st_info, st_other, st_shndx, st_value, st_size = struct.unpack_from("<IBBHQQ", blob, off + 24 * i)
        name = blob[stroff + st_name:blob.index(b"\0", stroff + st_name)].decode()
        if name:
            syms[name] = (st_value, st_size, st_shndx)
    return syms


MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib: str, tmp: str, tag: str):
    """The gfx950 code object of every translation unit: the linker concatenates one offload bundle per object file
    into .hip_fatbin."""
    blob = open(lib, "rb").read()
    off, size, _, _ = _sections(blob)[".hip_fatbin"]
    fat = blob[off:off + size]
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), fat)]
    out = []
    for i, s in enumerate(starts):
        path = os.path.join(tmp, f"{tag}.{i}")
        with open(path + ".bundle", "wb") as f:
            f.write(fat[s:starts[i + 1] if i + 1 < len(starts) else len(fat)])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", f"--targets={TARGET}",
                               f"--input={path}.bundle", f"--output={path}.co", "--unbundle"])
        out.append(path + ".co")
    return out


def all_kernels(lib: str, tmp: str, tag: str):
    ks = {}
    for co in code_objects(lib, tmp, tag):
        ks.update(kernels(co))
    return ks


def kernels(co: str):
    """{kernel: (disassembly lines, descriptor bytes)}"""
    blob = open(co, "rb").read()
    secs = _sections(blob)
    syms = _symbols(blob, secs)
    by_index = {i: s for i, s in enumerate(secs.values())}
    kds = {}
    for name, (value, size, shndx) in syms.items():
        if name.endswith(".kd") and size == 64:
            s_off, _, s_addr, _ = by_index[shndx]
            kd = bytearray(blob[s_off + value - s_addr:s_off + value - s_addr + 64])
            kd[16:24] = bytes(8)  # kernel_code_entry_byte_offset: where the code lies relative to the descriptor
            kds[name[:-3]] = bytes(kd)
    dis = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn",
                                   "--no-leading-addr", co], text=True)
    bodies, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^<(.+)>:$", line.strip())
        if m:
            cur = m.group(1)
            bodies[cur] = []
            continue
        if cur is None or not line.strip():
            continue
        bodies[cur].append(line.split("//")[0].strip())
    for body in bodies.values():  # "...": the zero padding up to the next symbol's alignment, not part of the kernel
        while body and body[-1] == "...":
            body.pop()
    return {k: (bodies.get(k, []), kd) for k, kd in kds.items()}


RES_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
            "private_segment_fixed_size", "group_segment_fixed_size")


def resources(lib: str, pattern: str):
    """{kernel: {key: int}} of the AMDGPU metadata (registers, spills, scratch, LDS) of the kernels matching `pattern`."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(lib, tmp, "res"):
            notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
            for block in re.split(r"\n  - \.", notes)[1:]:
                kv = dict(re.findall(r"^\s{0,4}\.?(\w+):\s+(\S+)\s*$", "." + block, flags=re.M))
                name = kv.get("name")
                if name and re.search(pattern, name):
                    out[name] = {k: int(kv[k]) for k in RES_KEYS if k in kv}
    return out


def opcode_diff(old_lines, new_lines):
    """'opcode old->new' for every opcode (first token of a disassembly line) whose count differs."""
    a = collections.Counter(l.split()[0] for l in old_lines if not l.endswith(":"))
    b = collections.Counter(l.split()[0] for l in new_lines if not l.endswith(":"))
    return " ".join(f"{op} {a[op]}->{b[op]}" for op in sorted(set(a) | set(b)) if a[op] != b[op])


def scalar_copies_reordered(old, new):
    """(lines, descriptor) pairs that differ only in where their s_mov_b32 / s_mov_b64 lines stand."""
    def rest(lines):
        return [l for l in lines if l.split()[0] not in ("s_mov_b32", "s_mov_b64")]

    return (old[1] == new[1] and collections.Counter(old[0]) == collections.Counter(new[0])
            and rest(old[0]) == rest(new[0]))


def main(argv):
    if len(argv) == 4 and argv[1] == "--resources":
        for k, v in sorted(resources(argv[2], argv[3]).items()):
            print(k, " ".join(f"{a}={b}" for a, b in v.items()))
        return 0
    opcodes = len(argv) == 4 and argv[1] == "--opcodes"
    if opcodes:
        argv = argv[:1] + argv[2:]
    if len(argv) != 3:
        print(__doc__)
        return 2
    with tempfile.TemporaryDirectory() as tmp:
        old = all_kernels(argv[1], tmp, "old")
        new = all_kernels(argv[2], tmp, "new")
    bad = reordered = 0
    for k in sorted(old):
        if k not in new:
            print("MISSING", k)
            bad += 1
        elif opcodes and old[k] != new[k] and scalar_copies_reordered(old[k], new[k]):
            print("REORDERED scalar copies", k)
            reordered += 1
        elif old[k] != new[k]:
            what = "descriptor" if old[k][1] != new[k][1] else "disassembly"
            print("CHANGED", what, k)
            if opcodes:
                print("   ", opcode_diff(old[k][0], new[k][0]) or "(every opcode count equal)")
            bad += 1
    added = sorted(set(new) - set(old))
    for k in added:
        print("new", k)
    print(f"{len(old)} kernels in the old build: {len(old) - bad - reordered} identical, "
          + (f"{reordered} with reordered scalar copies, " if opcodes else "") + f"{bad} differ; {len(added)} new")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

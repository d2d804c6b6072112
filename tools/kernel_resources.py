#!/usr/bin/env python3
"""Register / scratch / LDS figures of every kernel in a build directory, read from the code objects' metadata.

    tools/kernel_resources.py tmac_amd/csrc/build [--arch gfx950] [--filter k_gemv_stream] [--opcodes]

One line per kernel: demangled name | VGPRs, AGPRs, SGPRs, scratch bytes per lane (private_segment_fixed_size), static LDS bytes,
VGPR / SGPR spill counts.  Needs no GPU: it unbundles the device code object of each *.o (clang-offload-bundler) and reads its notes
(llvm-readelf).  Two listings made from two commits can be compared with diff(1); an added template argument shows in the names.
--opcodes adds, per kernel, the number of instructions and a short hash of the sequence of their mnemonics (llvm-objdump -d of the same
code object, operands dropped): between two commits, diff(1) then also shows which kernels the compiler scheduled differently.
"""
import argparse
import glob
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("TMAC_LLVM_BIN", "/opt/rocm/llvm/bin")
KEYS = [("vgpr_count", "VGPR"), ("agpr_count", "AGPR"), ("sgpr_count", "SGPR"), ("private_segment_fixed_size", "scratch"),
        ("group_segment_fixed_size", "LDS"), ("vgpr_spill_count", "vspill"), ("sgpr_spill_count", "sspill")]


def opcodes_of(co):
    """symbol -> (instruction count, hash of the mnemonic sequence) for every function of a code object"""
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], capture_output=True, text=True).stdout
    out, name, ops = {}, None, []
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            if name is not None:
                out[name] = (len(ops), hashlib.sha1(" ".join(ops).encode()).hexdigest()[:12])
            name, ops = m.group(1), []
        elif name is not None and line.startswith((" ", "\t")) and line.strip() and line.strip() != "...":
            # ("...": llvm-objdump's mark for zero padding behind a function -- where the next one starts, not what this one does)
            ops.append(line.split("//")[0].split()[0])
    if name is not None:
        out[name] = (len(ops), hashlib.sha1(" ".join(ops).encode()).hexdigest()[:12])
    return out


def kernels_of(obj, arch, tmp, opcodes=False):
    # the device code sits in the object's .hip_fatbin section as an offload bundle
    sec = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-S", "-W", obj], capture_output=True, text=True).stdout
    m = re.search(r"\.hip_fatbin\s+PROGBITS\s+[0-9a-f]+\s+([0-9a-f]+)\s+([0-9a-f]+)", sec)
    if not m:
        return []
    off, size = int(m.group(1), 16), int(m.group(2), 16)
    bundle, co = os.path.join(tmp, "bundle.bin"), os.path.join(tmp, "device.co")
    with open(obj, "rb") as f:
        f.seek(off)
        data = f.read(size)
    with open(bundle, "wb") as f:
        f.write(data)
    if os.path.exists(co):
        os.remove(co)
    r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", f"--targets=hipv4-amdgcn-amd-amdhsa--{arch}",
                        f"--input={bundle}", f"--output={co}", "--unbundle"], capture_output=True, text=True)
    if r.returncode != 0 or not os.path.exists(co) or os.path.getsize(co) == 0:
        return []
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True).stdout
    out, cur = [], None
    for line in notes.splitlines():
        first = re.match(r"^  - \.(\w+):\s*(.*)$", line)            # a kernel's map starts here; its own keys are indented by four
        m = first or re.match(r"^    \.(\w+):\s*(.*)$", line)
        if first:
            cur = {}
            out.append(cur)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2).strip().strip("'")
    out = [k for k in out if "name" in k]
    if opcodes:
        ops = opcodes_of(co)
        for k in out:
            k["insts"], k["ophash"] = ops.get(k["name"], ("?", "?"))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("build_dir")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--filter", default="", help="only kernels whose demangled name contains this")
    ap.add_argument("--opcodes", action="store_true", help="also print each kernel's instruction count and a hash of its mnemonic sequence")
    a = ap.parse_args()
    keys = KEYS + ([("insts", "insts"), ("ophash", "ops")] if a.opcodes else [])
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sorted(glob.glob(os.path.join(a.build_dir, "*.o"))):
            for k in kernels_of(obj, a.arch, tmp, a.opcodes):
                rows.append((os.path.basename(obj), k))
    filt = shutil.which("c++filt")
    names = [k["name"] for _, k in rows]
    dem = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True).stdout.split("\n") if filt and names else names
    lines = []
    for (obj, k), d in zip(rows, dem):
        if a.filter and a.filter not in d:
            continue
        lines.append(f"{obj}: {d} | " + " ".join(f"{lab} {k.get(key, '?')}" for key, lab in keys))
    print("\n".join(sorted(lines)))
    return 0


if __name__ == "__main__":
    sys.exit(main())

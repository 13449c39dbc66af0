#!/usr/bin/env python3
"""Is the gfx950 device code of two source trees the same, kernel by kernel? For a host-only refactor it has to be.

    python scripts/compare_device_code.py OLD_CSRC NEW_CSRC scatter density_mlp sampler ...

Builds the device-only code object of every named .hip file in both directories with the Makefile's flags and compares
  - the set of symbols (kernels, their descriptors, device functions and variables) with types and sizes, but for
    __hip_cuid_<hash>, which names the translation unit by a hash of its source,
  - every function's disassembly: mnemonics, operands and encodings, with branch targets as symbol + offset — so a kernel
    that merely moved inside the object (another instantiation order on the host side) compares equal,
  - every kernel descriptor (registers, LDS, scratch, enabled SGPRs, ...) but its offset to the kernel's entry.
Prints one line per file and exits non-zero on any difference.
"""
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LLVM = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "llvm", "bin")
HERE = os.path.dirname(os.path.abspath(__file__))


def makefile_flags():
    text = open(os.path.join(HERE, "..", "nerfstudio_amd", "csrc", "Makefile")).read()
    flags = re.search(r"^FLAGS\s*:=\s*(.*)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)).split()


def build(src_dir, name, out):
    cmd = [HIPCC] + makefile_flags() + ["--cuda-device-only", "--no-gpu-bundle-output", "-c", name + ".hip", "-o", out]
    return subprocess.Popen(cmd, cwd=src_dir), " ".join(cmd)


def functions(obj):
    """{symbol: [instruction lines without addresses]}"""
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", obj], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t") and line.strip() != "...":  # ("...": zero padding behind a function)
            cur.append(re.sub(r"// [0-9A-F]+:", "//", line))
    return out


def symbols_and_descriptors(obj):
    """(sorted [(name, type, size)], {kernel descriptor symbol: its 64 bytes without the entry offset})"""
    text = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-s", "-S", "-W", obj], check=True, capture_output=True, text=True).stdout
    sections = {}
    for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", text, re.M):
        sections[int(m.group(1))] = (int(m.group(3), 16), int(m.group(4), 16))  # address, file offset
    syms, kds = set(), {}
    data = open(obj, "rb").read()
    for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+(\S+)\s+\S+\s+\S+\s+(\d+)\s+(\S+)$", text, re.M):
        value, size, kind, ndx, name = int(m.group(1), 16), int(m.group(2)), m.group(3), int(m.group(4)), m.group(5)
        if not name.startswith("__hip_cuid_"):  # the translation unit's id: a hash of its whole source, host code included
            syms.add((name, kind, size))
        if name.endswith(".kd"):
            addr, off = sections[ndx]
            kd = data[off + value - addr:off + value - addr + 64]
            kds[name] = kd[:16] + kd[24:]  # bytes 16-23: kernel_code_entry_byte_offset
    return sorted(syms), kds


def main():
    old, new, names = sys.argv[1], sys.argv[2], sys.argv[3:]
    tmp = tempfile.mkdtemp(prefix="devcmp_")
    jobs = []
    for n in names:
        for side, d in (("old", old), ("new", new)):
            jobs.append(build(d, n, os.path.join(tmp, f"{n}.{side}.o")))
    print("# " + jobs[0][1].replace(names[0] + ".hip", "<file>.hip").replace(os.path.join(tmp, names[0] + ".old.o"), "<file>.o"))
    if any(p.wait() != 0 for p, _ in jobs):
        sys.exit("build failed")
    bad = 0
    for n in names:
        o, w = os.path.join(tmp, f"{n}.old.o"), os.path.join(tmp, f"{n}.new.o")
        fo, fw = functions(o), functions(w)
        (so, ko), (sw, kw) = symbols_and_descriptors(o), symbols_and_descriptors(w)
        differing = sorted(k for k in set(fo) | set(fw) if fo.get(k) != fw.get(k))
        same_order = list(fo) == list(fw)
        ok = so == sw and not differing and ko == kw
        bad += not ok
        print(f"{n}.hip: {len(ko)} kernels, {len(fo)} functions, {sum(map(len, fw.values()))} instructions: "
              f"symbols {'identical' if so == sw else 'DIFFER'}, per-function disassembly {'identical' if not differing else 'DIFFERS'}, "
              f"kernel descriptors {'identical' if ko == kw else 'DIFFER'}, order in the object {'same' if same_order else 'permuted'}")
        for k in differing[:10]:
            print("    differs:", k)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

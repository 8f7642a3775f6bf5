#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of libx264hip.so instruction by instruction (no GPU):
the disassembly of tests/test_codegen.py, addresses and encodings dropped.

    python tools/codegen_diff.py [--sub PATTERN REPL] OLD.so NEW.so [name substring ...]

Prints, for every kernel whose name holds one of the substrings (default: all), whether its
instruction stream is identical, and for those that differ or exist in one build only the
instruction counts and the VGPR / SGPR / scratch / LDS figures of both kernel descriptors."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _tool(name):
    p = os.path.join(LLVM, name)
    return p if os.path.exists(p) else shutil.which(name)


def kernels(so):
    """{kernel: ([instructions], {resource: value})}"""
    objcopy, bundler, objdump, readelf = (_tool(t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump",
                                                               "llvm-readelf"))
    out = {}
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.run([objcopy, "--dump-section", f".hip_fatbin={fat}", so, os.path.join(d, "so.tmp")], check=True,
                       capture_output=True)
        data = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
        for i, s in enumerate(starts):
            e = starts[i + 1] if i + 1 < len(starts) else len(data)
            chunk, co = os.path.join(d, f"b{i}.bin"), os.path.join(d, f"b{i}.co")
            open(chunk, "wb").write(data[s:e])
            r = subprocess.run([bundler, "--unbundle", "--type=o", f"--input={chunk}",
                                "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], capture_output=True)
            if r.returncode or not os.path.exists(co) or os.path.getsize(co) == 0:
                continue
            dis = subprocess.run([objdump, "-d", co], capture_output=True, text=True, check=True).stdout
            name = None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
                if m:
                    name = m.group(1)
                    out.setdefault(name, ([], {}))
                elif name and line.startswith("\t") and line.strip() != "...":    # (not the padding after a kernel)
                    out[name][0].append(line.split("//")[0].strip())
            notes = subprocess.run([readelf, "--notes", co], capture_output=True, text=True).stdout
            # a kernel's metadata block runs from its .agpr_count (the first key) to the next one
            blk = {}
            for line in notes.splitlines() + ["- .agpr_count: 0"]:
                m = re.match(r"\s*(-?)\s*\.(\w+):\s*(\S+)", line)
                if not m:
                    continue
                dash, k, v = m.groups()
                if k == "agpr_count" and dash:
                    if blk.get("symbol", "")[:-3] in out:
                        out[blk["symbol"][:-3]][1].update({q: blk[q] for q in ("vgpr_count", "sgpr_count", "agpr_count",
                                                                               "private_segment_fixed_size",
                                                                               "group_segment_fixed_size") if q in blk})
                    blk = {}
                blk.setdefault(k, v)
    return out


def main():
    args = sys.argv[1:]
    rename = None
    if "--sub" in args:                  # --sub PATTERN REPL: rewrite the kernel names of both builds first
        i = args.index("--sub")
        rename = (re.compile(args[i + 1]), args[i + 2])
        del args[i:i + 3]
    old, new = kernels(args[0]), kernels(args[1])
    if rename:
        old = {rename[0].sub(rename[1], k): v for k, v in old.items()}
        new = {rename[0].sub(rename[1], k): v for k, v in new.items()}
    subs = args[2:]
    same = 0
    for k in sorted(set(old) | set(new)):
        if subs and not any(s in k for s in subs):
            continue
        if k in old and k in new and old[k][0] == new[k][0]:
            same += 1
            continue
        a = f"{len(old[k][0])} instr {old[k][1]}" if k in old else "absent"
        b = f"{len(new[k][0])} instr {new[k][1]}" if k in new else "absent"
        print(f"{k}\n    old: {a}\n    new: {b}")
    print(f"{same} kernels with identical instruction streams")


if __name__ == "__main__":
    main()

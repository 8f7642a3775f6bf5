#!/usr/bin/env python3
"""Per-kernel differences of two device assembly listings: isa_diff.py <old.s> <new.s>

The listings come from e.g.  hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S file.hip
For every kernel whose opcode counts or resources differ it prints the opcode-count differences
(all, and with s_nop / s_waitcnt left out) and the changes of .vgpr_count, .sgpr_count,
.private_segment_fixed_size and the spill counts; then the two files' symbol-set difference.
It compares counts only.  Exit status 1 when a kernel's counts differ beyond s_nop / s_waitcnt
or the symbol sets differ.
"""
import collections, re, sys

PAD = ("s_nop", "s_waitcnt")
KEYS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".sgpr_spill_count", ".vgpr_spill_count")


def parse(path):
    s = open(path).read()
    hist, meta = {}, {}
    for m in re.finditer(r"^(_Z\S+):.*?^\.Lfunc_end", s, re.M | re.S):
        lines = (l.strip() for l in m.group(0).split("\n")[1:])
        hist[m.group(1)] = collections.Counter(
            l.split()[0] for l in lines if l and not l.startswith((";", ".", "_Z")) and not l.split()[0].endswith(":"))
    for blk in s[s.find("amdhsa.kernels:"):].split("  - .")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name:
            meta[name.group(1)] = {k: int(re.search(re.escape(k) + r":\s+(\d+)", blk).group(1)) for k in KEYS}
    return hist, meta


def delta(a, b, skip=()):
    return {k: (a[k], b[k]) for k in sorted(set(a) | set(b)) if a[k] != b[k] and k not in skip}


def main():
    (ha, ma), (hb, mb) = parse(sys.argv[1]), parse(sys.argv[2])
    same = padding = moved = 0
    for name in sorted(set(ha) & set(hb)):
        full, core = delta(ha[name], hb[name]), delta(ha[name], hb[name], PAD)
        res = {k: (ma[name][k], mb[name][k]) for k in KEYS if name in ma and name in mb and ma[name][k] != mb[name][k]}
        if not full and not res:
            same += 1
            continue
        padding += not core
        moved += bool(core)
        fmt = lambda d: "  ".join(f"{k}:{x}->{y}" for k, (x, y) in d.items()) or "equal"
        print(name)
        print("  opcodes:", fmt(full))
        print("  without s_nop/s_waitcnt:", fmt(core))
        print("  resources:", fmt(res))
    only_a, only_b = sorted(set(ha) - set(hb)), sorted(set(hb) - set(ha))
    for n in only_a:
        print("only in", sys.argv[1] + ":", n)
    for n in only_b:
        print("only in", sys.argv[2] + ":", n)
    print(f"{len(ha)} / {len(hb)} symbols, {len(only_a) + len(only_b)} unmatched; {same} kernels with equal counts, "
          f"{padding} differ in s_nop/s_waitcnt or resources only, {moved} differ in other opcodes")
    return 1 if moved or only_a or only_b else 0


if __name__ == "__main__":
    sys.exit(main())

"""Per-kernel comparison of two device assembly listings (developer tool): did a source change alter a kernel's code object?
usage: hipcc <build flags> --cuda-device-only -S file.hip -o a.s   (both versions) ; python tools/isa_diff.py a.s b.s [name substring] [OLD=NEW ...]
OLD=NEW pairs a kernel that the change renamed: substrings of the mangled names in a.s and b.s, each matching exactly one kernel.
Per kernel: IDENTICAL (same instruction stream), REGS (same opcode sequence, other register numbers / operands) or DIFFERENT; the
instruction counts; vgpr / vgpr spill / sgpr spill / private segment from the metadata; for changed kernels whether the hand-written
(inline asm) s_waitcnt immediates are the same multiset, else what each side has more of."""
import collections
import re
import subprocess
import sys

META = (".vgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size")


def kernels(path):
    text = open(path).read()
    meta = {}
    for blk in re.split(r"\n  - \.agpr_count:", text.split(".amdgpu_metadata")[-1])[1:]:
        name = re.search(r"\n    \.name:\s+(\S+)", blk).group(1)
        meta[name] = [int(re.search(r"\n    \%s:\s+(\d+)" % k, blk).group(1)) for k in META]
    out = {}
    for name in meta:
        body = text.split("\n%s:" % name, 1)[1].split("\n.Lfunc_end", 1)[0]
        ins = [re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0].strip()) for l in body.split("\n") if l.startswith("\t") and not l.startswith("\t.")]
        hand = re.findall(r"#ASMSTART\n\ts_waitcnt ([^\n]*)", body)
        out[name] = ([i for i in ins if i], meta[name], collections.Counter(hand))
    return out


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
want = "".join(x for x in sys.argv[3:] if "=" not in x)
for old, new in (x.split("=") for x in sys.argv[3:] if "=" in x):        # a renamed kernel goes by its old name on both sides
    (o,), (n,) = [k for k in a if old in k], [k for k in b if new in k]
    b = {(o if k == n else k): v for k, v in b.items()}
names = [n for n in a if want in n] + [n for n in b if n not in a and want in n]
try:
    pretty = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")))
except OSError:
    pretty = {}
print("%-9s %-52s %13s  %s" % ("result", "kernel", "instructions", "vgpr/vspill/sspill/private"))
for n in names:
    if n not in a or n not in b:
        print("%-9s %s" % ("ONLY-A" if n in a else "ONLY-B", pretty.get(n, n)))
        continue
    (ia, ma, wa), (ib, mb, wb) = a[n], b[n]
    res = "IDENTICAL" if ia == ib else ("REGS" if [i.split()[0] for i in ia] == [i.split()[0] for i in ib] else "DIFFERENT")
    short = re.sub(r"\(anonymous namespace\)::|\(.*", "", pretty.get(n, n))
    line = "%-9s %-52s %6d %6d  %s -> %s" % (res, short[:52], len(ia), len(ib), "/".join(map(str, ma)), "/".join(map(str, mb)))
    if res != "IDENTICAL":
        line += "  asm waits " + ("same" if wa == wb else "A-B %s B-A %s" % (dict(wa - wb), dict(wb - wa)))
    print(line)

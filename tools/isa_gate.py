"""The ISA gate of a refactor: compare the device assembly of two builds of the library, kernel by kernel.

    hipcc -O3 --offload-arch=gfx950 -std=c++17 -w --cuda-device-only -S vjf_amd/csrc/vjf_abi.hip -o FILE.s     (in each tree)
    python tools/isa_gate.py PARENT.s BRANCH.s

Per kernel: codeLenInByte / NumVgprs / TotalNumSgprs / ScratchSize (bytes per lane) / count of v_writelane + v_readlane (SGPRs
spilled into VGPR lanes) / instruction lines, for both files where they differ, and "diff" = the number of instruction lines that
differ once comments, labels and directives are stripped, branch-target labels are renumbered to one name and the immediates of
scalar s_mov_b32 / s_movk_i32 / s_cmp_* / s_cmpk_* / s_cselect_b32 are masked (the selector constants the compiler numbers the
inlined call sites with); "n/a" where the line counts differ; "window" = the lines of parent / branch between the kernels' common
head and common tail (where the code moved: one line inserted shifts every line behind it in "diff").  Each kernel is put into a tier (profiles/mega_split_isa.txt):
    A      the four resource figures and the lane-spill count equal, diff 0
    B      code moves, but VGPRs, scratch and the lane-spill count are not above the parent's
    drop   anything else
It compares two files; it searches them for nothing.  Exit code: 0 all tier A, 1 some tier B, 2 some kernel beyond tier B.
"""
import re
import sys

FIGURES = (("code", r";\s*codeLenInByte\s*=\s*(\d+)"), ("vgpr", r";\s*NumVgprs:\s*(\d+)"), ("sgpr", r";\s*TotalNumSgprs:\s*(\d+)"),
           ("scratch", r";\s*ScratchSize:\s*(\d+)"))
MASKED = re.compile(r"^(s_mov_b32|s_movk_i32|s_cmp_\w+|s_cmpk_\w+|s_cselect_b32)\s")
IMM = re.compile(r"(?<![\w.])(-?0x[0-9a-fA-F]+|-?\d+)(?![\w.])")


def short_name(sym):
    m = re.match(r"_Z(?:N12_GLOBAL__N_1)?(\d+)", sym)             # (kernels of an anonymous namespace keep their plain name)
    if not m:
        return sym
    n = int(m.group(1))
    name, rest = sym[m.end():m.end() + n], sym[m.end() + n:]
    t = re.match(r"I((?:L[a-z]\d+E)+)E", rest)
    if t:
        name += "<" + ",".join(re.findall(r"L[a-z](\d+)E", t.group(1))) + ">"
    return name


def normalise(line):
    t = line.split(";")[0].strip()
    if not t or t.startswith(".") or t.endswith(":"):
        return None
    t = re.sub(r"\.LBB\d+_\d+", ".L", t)
    if MASKED.match(t):
        op, _, args = t.partition(" ")
        t = op + " " + IMM.sub("#", args)
    return re.sub(r"\s+", " ", t)


def kernels(path):
    src = open(path).read().split("\n")
    out, order = {}, []
    i = 0
    while i < len(src):
        m = re.match(r"\s*\.type\s+(\S+),@function", src[i])
        if not m:
            i += 1
            continue
        sym = m.group(1)
        while i < len(src) and not src[i].startswith(sym + ":"):
            i += 1
        body = []
        i += 1
        while i < len(src) and not re.match(r"\s*\.section\s|\.Lfunc_end", src[i]):
            t = normalise(src[i])
            if t is not None:
                body.append(t)
            i += 1
        k = {"lines": body, "spill": sum(1 for t in body if t.startswith(("v_writelane", "v_readlane")))}
        while i < len(src) and not re.match(r";\s*codeLenInByte", src[i]):
            i += 1
        for j in range(i, min(i + 12, len(src))):
            for key, pat in FIGURES:
                f = re.match(pat, src[j])
                if f and key not in k:
                    k[key] = int(f.group(1))
        if all(key in k for key, _ in FIGURES):      # (device functions that are not kernels carry no "Kernel info")
            out[sym] = k
            order.append(sym)
    return out, order


def window(a, b):
    head = 0
    while head < min(len(a), len(b)) and a[head] == b[head]:
        head += 1
    tail = 0
    while tail < min(len(a), len(b)) - head and a[-1 - tail] == b[-1 - tail]:
        tail += 1
    return head, len(a) - head - tail, len(b) - head - tail


def figures(k):
    return f"{k['code']:>7} / {k['vgpr']:>3} / {k['sgpr']:>3} / {k['scratch']:>3} / {k['spill']:>4} / {len(k['lines']):>5}"


def main(argv):
    if len(argv) != 2:
        print(__doc__)
        return 2
    (ka, order), (kb, order_b) = kernels(argv[0]), kernels(argv[1])
    worst, tiers = 0, {"A": 0, "B": 0, "drop": 0}
    width = max(len(short_name(s)) for s in order + order_b)
    for sym in order + [s for s in order_b if s not in ka]:
        a, b = ka.get(sym), kb.get(sym)
        if a is None or b is None:
            print(f"  {short_name(sym):<{width}}  only in the {'branch' if a is None else 'parent'}")
            tiers["drop"] += 1
            worst = 2
            continue
        same = len(a["lines"]) == len(b["lines"])
        diff = sum(1 for x, y in zip(a["lines"], b["lines"]) if x != y) if same else None
        equal = all(a[key] == b[key] for key in ("code", "vgpr", "sgpr", "scratch", "spill"))
        if equal and diff == 0:
            tier = "A"
        elif all(b[key] <= a[key] for key in ("vgpr", "scratch", "spill")):
            tier = "B"
        else:
            tier = "drop"
        tiers[tier] += 1
        worst = max(worst, {"A": 0, "B": 1, "drop": 2}[tier])
        print(f"  {short_name(sym):<{width}}  {figures(a)}" + ("" if equal and same else f"  ->  {figures(b)}") +
              f"   diff {'n/a' if diff is None else diff}" + ("" if diff == 0 else "   window %d / %d" % window(a["lines"], b["lines"])[1:]) + f"   tier {tier}")
    print(f"{len(order)} kernels in the parent, {len(order_b)} in the branch: tier A {tiers['A']}, tier B {tiers['B']}, beyond {tiers['drop']}")
    return worst


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

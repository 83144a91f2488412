"""Development aid (no GPU): instruction mix of the backward sweep's stage block of a compiled column kernel — the basic block
with the most `v_fmac_f64_dpp` (the row-paired stage loop's main block) — plus the symbol's VGPRs and scratch bytes.

    python tools/stage_block.py <kernel.s> <symbol prefix> [<symbol prefix> ...] [--brief]      (see tools/asm_loops.py for the compile line)

Every symbol that starts with one of the prefixes is listed; --brief prints one line of selected counts per symbol.

VALU = every `v_*` instruction of the block; the table lists each mnemonic that occurs (docs/PIVOT_STEP.md).
"""
import collections
import re
import sys


def blocks(lines):
    cur = []
    for l in lines:
        s = l.strip()
        if re.match(r"\.LBB\d+_\d+:", s):
            yield cur
            cur = []
        elif s and not s.startswith((".", ";")) and not s.endswith(":"):
            cur.append(s.split()[0])
            if s.startswith(("s_cbranch", "s_branch")):
                yield cur
                cur = []
    yield cur


def main():
    f = open(sys.argv[1]).read().split("\n")
    args = [a for a in sys.argv[2:] if a != "--brief"]
    brief = "--brief" in sys.argv
    for start in [i for i, l in enumerate(f) if l.endswith(":") and any(l.startswith(a) for a in args)] \
            + [i for i, l in enumerate(f) if ": " in l and l.split(":")[0].startswith(tuple(args)) and not l.startswith((" ", "\t", ";", "."))]:
        end = [i for i, l in enumerate(f) if i > start and l.startswith(".Lfunc_end")][0]
        name = f[start].split()[0].rstrip(":")
        meta = {}
        for l in f[end:]:
            m = re.match(r"\s*\.(vgpr_count|private_segment_fixed_size|name):\s+(\S+)", l)
            if m:
                meta[m.group(1)] = m.group(2)
                if m.group(1) == "vgpr_count" and meta.get("name") == name:
                    break
        best = max(blocks(f[start:end]), key=lambda b: sum(x == "v_fmac_f64_dpp" for x in b))
        c = collections.Counter(best)
        valu = sum(n for k, n in c.items() if k.startswith("v_"))
        print("%s: vgprs %s scratch %s | stage block %d instructions, %d VALU" % (name, meta.get("vgpr_count"), meta.get("private_segment_fixed_size"), len(best), valu))
        if brief:
            keys = ("v_fmac_f64_dpp", "v_fmac_f64_e32", "v_fma_f64", "v_mul_f64", "v_add_f64", "v_rcp_f64_e32", "v_cmp_gt_f64_e32", "v_cmp_gt_f64_e64",
                    "v_cndmask_b32_e32", "v_cndmask_b32_e64", "v_mov_b32_e32", "v_mov_b64_e32", "v_readlane_b32", "s_nop")
            print("    " + ", ".join("%s %d" % (k, c.get(k, 0)) for k in keys))
            continue
        for k, n in sorted(c.items(), key=lambda kv: (-kv[1], kv[0])):
            print("    %-28s %4d" % (k, n))


if __name__ == "__main__":
    main()

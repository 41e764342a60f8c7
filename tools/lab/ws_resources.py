#!/usr/bin/env python3
"""Resource table of fused_layer_ws_kernel's instantiations from the compiler's metadata of two builds.

  hipcc <csrc/Makefile's FLAGS> --save-temps -c csrc/fused_layer_ws.hip      # once per build, in its own directory
  python tools/lab/ws_resources.py BEFORE.s AFTER.s > profiles/NAME.txt

Reads the amdhsa.kernels metadata of the two gfx950 assembly files (.vgpr_count, .private_segment_fixed_size = scratch
bytes per lane, .group_segment_fixed_size = LDS bytes) and the kernel bodies (scratch_ instructions, LDS-DMA loads,
`s_waitcnt vmcnt(0)` between the first LDS-DMA load and the kernel's end, i.e. in the producers' code; that the
counted wait ahead of the raw barrier has the count the source derives and no register load sits behind that barrier).
Waves per SIMD: the smaller of the compiler's "Occupancy" and what the LDS footprint allows.  Exit status 1 if an instantiation's
scratch grew, its waves per SIMD changed or the order check failed.
"""
import re
import sys

NAME = re.compile(r"fused_layer_ws_kernelI((?:L[ib]\d+E)+)E")


def template_args(mangled):
    m = NAME.search(mangled)
    if not m:
        return None
    return tuple(int(v) for v in re.findall(r"L[ib](\d+)E", m.group(1)))


def label(a):
    rt, ct, wr, wc, kc, radd, gath, split, pool, pair = a
    form = {0: "plain", 1: "ball", 2: "knn"}[gath]
    if radd:
        form = "res" if gath == 0 else "res-" + form + "-gathered (RG)"
    form += " split" if split else ""
    form += " pool" if pool else ""
    form += " pair" if pair else ""
    return "%3dx%-3d kc%-2d %s" % (wr * rt * 32, wc * ct * 32, kc, form)


def waves(k):
    # whole 8-wave workgroups (2 waves per SIMD each): what the registers (the compiler's figure) and 160 KB of LDS
    # per CU allow
    return 2 * min(k["waves"] // 2, 160 * 1024 // k["lds"])


def expected_counts(a):
    """(NVM, NVM_G) of the producers' loop in fused_layer_ws.hip for template arguments a."""
    rt, ct, wr, wc, kc, radd, gath, split, pool, pair = a
    apt4 = wr * rt * 32 // (256 // (kc // 4))
    rg = radd and gath != 0
    nvm = 3 + apt4 + (apt4 if radd else 0) + ((1 + (2 if gath == 2 else 0)) if rg else 0)
    return nvm, nvm + 1 + (2 if gath == 2 else 0)


def order_faults(a, body):
    """What would break the counted wait: a wait of another count, or a register load that the compiler moved from
    before the raw barrier to behind it (it would sit between the DMA and the wait that counts on its absence)."""
    faults = []
    want = sorted(set(expected_counts(a)[:2 if a[6] else 1]))
    got = sorted(set(int(n) for n in re.findall(r"s_waitcnt vmcnt\((\d+)\) lgkmcnt\(0\)\n", body)))
    if got != want:
        faults.append("wait counts %s, expected %s" % (got, want))
    # the rest of the barrier's basic block (up to the next label): the way to the DMA of the next chunk
    for m in re.finditer(r"s_waitcnt vmcnt\(\d+\) lgkmcnt\(0\)\n(?:[^\n]*\n){0,8}?\s+s_barrier\n(.*?)^\.LBB", body, re.M | re.S):
        if re.search(r"^\s+(global|buffer|flat)_load_dword", m.group(1), re.M):
            faults.append("register load between the raw barrier and the DMA")
    return faults


def read(path):
    text = open(path).read()
    out = {}
    # metadata
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        a = template_args(name)
        if a is None:
            continue
        out[a] = {
            "vgpr": int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1)),
            "scratch": int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)),
            "lds": int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1)),
        }
    # bodies
    for m in re.finditer(r"^(_ZN\S*fused_layer_ws_kernel\S+):[^\n]*\n(.*?)^; Occupancy: (\d+)", text, re.M | re.S):
        a = template_args(m.group(1))
        if a not in out:
            continue
        body = m.group(2)
        out[a]["waves"] = int(m.group(3))
        out[a]["scratch_ins"] = len(re.findall(r"^\s+scratch_", body, re.M))
        out[a]["dma"] = len(re.findall(r"^\s+global_load_lds_dwordx4", body, re.M))
        first = body.find("global_load_lds_dwordx4")
        out[a]["vm0"] = len(re.findall(r"s_waitcnt[^\n]*vmcnt\(0\)", body[first:])) if first >= 0 else 0
        out[a]["faults"] = order_faults(a, body) if first >= 0 else []
    return out


def main():
    before, after = read(sys.argv[1]), read(sys.argv[2])
    bad = 0
    print("fused_layer_ws_kernel, gfx950: before -> after (VGPRs | scratch bytes per lane | scratch instructions | "
          "LDS bytes | waves per SIMD | LDS-DMA loads | vmcnt(0) waits after the first LDS-DMA load)")
    for a in sorted(after, key=label):
        b, c = before.get(a), after[a]
        if b is None:
            print("%-44s new" % label(a))
            continue
        wb, wc = waves(b), waves(c)
        flag = ""
        if c["scratch"] > b["scratch"]:
            flag += "  SCRATCH GREW"
        if wb != wc:
            flag += "  WAVES CHANGED"
        for f in c.get("faults", []):
            flag += "  ORDER: " + f
        bad += bool(flag)
        print("%-44s %3d -> %3d | %3d -> %3d | %3d -> %3d | %5d -> %5d | %d -> %d | %2d | %d%s" % (
            label(a), b["vgpr"], c["vgpr"], b["scratch"], c["scratch"], b.get("scratch_ins", 0), c.get("scratch_ins", 0),
            b["lds"], c["lds"], wb, wc, c.get("dma", 0), c.get("vm0", 0), flag))
    tot_b = sum(v.get("scratch_ins", 0) for v in before.values())
    tot_c = sum(v.get("scratch_ins", 0) for v in after.values())
    print("scratch_ instructions in all instantiations: %d -> %d" % (tot_b, tot_c))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Where the scratch instructions of the f16x3 kernels sit, read from the gfx950 assembly hipcc leaves with --save-temps
(`make -C groupnet_amd/csrc spills` writes it and runs this file on it).

An f16x3 kernel (P = 2) carries two bodies: the fp16 chain (v_mfma_f32_32x32x16_f16) and, behind the workgroup's range
vote, the bf16x6 fallback (v_mfma_f32_32x32x16_bf16), which in-range data never executes.  Compiled for three waves per
SIMD the kernels fit 168 registers only with spills, and the spills belong in the fallback.  For every kernel that issues
fp16 MFMAs this reports

  vgprs, scratch bytes per lane, static LDS, occupancy (waves per SIMD)      from the kernel descriptor and remarks
  scratch_load / scratch_store instructions before, inside and behind the     in the order of the listing
      span from the first to the last fp16 MFMA
  ... on the HOT paths: in a basic block that lies on some path from the       from the control-flow graph of the listing
      kernel's entry to an s_endpgm which passes through no block with a bf16
      MFMA — the paths a workgroup can take without falling back

usage: spill_regions.py LISTING.s [--json]
"""
import json
import re
import sys

F16 = "v_mfma_f32_32x32x16_f16"
BF16 = "v_mfma_f32_32x32x16_bf16"
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^\s+(s_branch|s_cbranch_\w+)\s+(\.LBB\d+_\d+)")


def kernels(text):
    """{mangled name: lines of the function body} for every function of the listing."""
    out, name, body = {}, None, []
    for line in text.splitlines():
        m = re.match(r"^(\w+):\s+; @\1", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name], name = body, None
            else:
                body.append(line)
    return out


def descriptor(text, name):
    """Fields of the .amdhsa_kernel block and the resource comments behind the function."""
    d = {}
    m = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", text, flags=re.S)
    if m:
        for key, field in (("lds", "group_segment_fixed_size"), ("scratch", "private_segment_fixed_size"),
                           ("vgprs", "next_free_vgpr")):
            f = re.search(r"\.amdhsa_" + field + r"\s+(\d+)", m.group(1))
            if f:
                d[key] = int(f.group(1))
    m = re.search(r"\.set " + re.escape(name) + r"\.num_vgpr, (\d+)", text)
    if m:
        d["vgprs"] = int(m.group(1))
    m = re.search(re.escape(name) + r":.*?\n; Occupancy: (\d+)", text, flags=re.S)
    if m:
        d["occupancy"] = int(m.group(1))
    return d


def blocks(body):
    """Basic blocks of a function body: [(label or None, [instruction lines])], split at labels and behind branches."""
    out, cur, label = [], [], None
    for line in body:
        m = LABEL.match(line)
        if m:
            out.append((label, cur))
            cur, label = [], m.group(1)
            continue
        code = line.split(";")[0].rstrip()
        if not code.strip() or code.lstrip().startswith("."):
            continue
        cur.append(code.strip())
        if BRANCH.match(code) or code.strip().startswith("s_endpgm"):
            out.append((label, cur))
            cur, label = [], None
    out.append((label, cur))
    return out


def analyse(body):
    bl = blocks(body)
    index = {lab: i for i, (lab, _) in enumerate(bl) if lab}
    succ = [[] for _ in bl]
    for i, (_, ins) in enumerate(bl):
        last = ins[-1] if ins else ""
        if any(w in x for x in ins for w in ("s_setpc", "s_swappc")):
            raise ValueError("indirect control flow: the hot-path analysis does not cover it")
        m = BRANCH.match("\t" + last)
        if m:
            succ[i].append(index[m.group(2)])
        if not last.startswith(("s_branch", "s_endpgm")) and i + 1 < len(bl):
            succ[i].append(i + 1)
    cold = [any(x.startswith(BF16) for x in ins) for _, ins in bl]
    ends = [i for i, (_, ins) in enumerate(bl) if ins and ins[-1].startswith("s_endpgm")]

    def reach(starts, edges):
        seen, todo = set(), [s for s in starts if not cold[s]]
        while todo:
            i = todo.pop()
            if i in seen:
                continue
            seen.add(i)
            todo += [j for j in edges[i] if not cold[j]]
        return seen

    pred = [[] for _ in bl]
    for i, ss in enumerate(succ):
        for j in ss:
            pred[j].append(i)
    hot = reach([0], succ) & reach(ends, pred)
    flat = [(i, x) for i, (_, ins) in enumerate(bl) for x in ins]
    f16 = [k for k, (_, x) in enumerate(flat) if x.startswith(F16)]
    res = {"fp16_mfma": len(f16), "bf16_mfma": sum(x.startswith(BF16) for _, x in flat),
           "before": 0, "inside": 0, "behind": 0, "hot": 0, "hot_before": 0}
    if not f16:
        return res
    for k, (i, x) in enumerate(flat):
        if not x.startswith(("scratch_load", "scratch_store")):
            continue
        where = "before" if k < f16[0] else ("inside" if k <= f16[-1] else "behind")
        res[where] += 1
        if i in hot:
            res["hot"] += 1
            res["hot_before"] += where == "before"
    return res


def report(path):
    text = open(path).read()
    out = {}
    for name, body in kernels(text).items():
        if not any(F16 in line for line in body):
            continue
        r = analyse(body)
        if r["fp16_mfma"]:
            r.update(descriptor(text, name))
            out[name] = r
    return out


def main(argv):
    if len(argv) < 2:
        raise SystemExit(__doc__)
    rep = report(argv[1])
    if "--json" in argv:
        print(json.dumps(rep, indent=1))
        return
    print(f"{'kernel':70s} vgpr scratch   lds occ | scratch instr.: before inside behind | hot paths (before span)")
    for name, r in rep.items():
        print(f"{name[:70]:70s} {r.get('vgprs', -1):4d} {r.get('scratch', -1):7d} {r.get('lds', -1):5d} "
              f"{r.get('occupancy', -1):3d} | {r['before']:22d} {r['inside']:6d} {r['behind']:6d} | {r['hot']:4d} ({r['hot_before']})")


if __name__ == "__main__":
    main(sys.argv)

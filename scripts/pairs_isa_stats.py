#!/usr/bin/env python3
"""Register and instruction figures of every pgx_find_mems_pairs_kernel instance, from the device assembly of pgx_pairs_kernels.hip
(hipcc -O3 --offload-arch=gfx950 -S --cuda-device-only): the code object's metadata (registers, spills, scratch, static LDS) and the instruction
mix of the whole body and of the main loop (from the first `s_setprio 3` to the last branch back to the label in front of it).
Usage: pairs_isa_stats.py <device .s file>; tests/test_pairs_kernel_resources.py imports stats()."""
import re
import sys

sys.path.insert(0, __file__.rsplit("/", 1)[0])
import isa_extract as I  # noqa: E402

META_KEYS = ("sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size", "kernarg_segment_size")


def metadata(path):
    """{kernel name: {key: int}} from the amdhsa.kernels list at the end of the file"""
    txt = open(path).read()
    at = txt.find("amdhsa.kernels:")
    out = {}
    if at < 0:
        return out
    for entry in re.split(r"\n  - ", txt[at:])[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry)
        if not name:
            continue
        d = {}
        for key in META_KEYS:
            m = re.search(r"\.%s:\s+(\d+)" % key, entry)
            if m:
                d[key] = int(m.group(1))
        out[name.group(1)] = d
    return out


def instructions(lines):
    out = []
    for ln in lines:
        s = ln.strip()
        if not s or s.startswith((";", ".", "//")) or s.endswith(":"):
            continue
        out.append(s)
    return out


def loop_of(lines):
    """the lines of the main loop: from the first s_setprio 3 to the last branch back to a label next to it (the compiler rotates the loop: the
    head's label stands up to a few instructions before or behind the s_setprio)"""
    first = next((i for i, ln in enumerate(lines) if ln.strip().startswith("s_setprio 3")), None)
    if first is None:
        return []
    heads = set()
    for i in range(max(first - 24, 0), min(first + 24, len(lines))):
        m = re.match(r"^(\.LBB\w+):", lines[i])
        if m:
            heads.add(m.group(1))
    last = first
    for i in range(first + 24, len(lines)):
        s = lines[i].strip()
        if s.startswith(("s_cbranch", "s_branch")) and s.split()[-1] in heads:
            last = i
    return lines[first:last + 1]


def count(lines):
    ins = instructions(lines)
    ops = [s.split()[0] for s in ins]
    return {
        "vector": sum(1 for o in ops if o.startswith("v_")),
        "scalar": sum(1 for o in ops if o.startswith("s_") and not o.startswith(("s_waitcnt", "s_load", "s_buffer_load"))),
        "s_load": sum(1 for o in ops if o.startswith(("s_load", "s_buffer_load"))),
        "v_readlane": sum(1 for o in ops if o.startswith("v_readlane_b32")),
        "v_writelane": sum(1 for o in ops if o.startswith("v_writelane_b32")),
        "s_mov": sum(1 for o in ops if o.startswith("s_mov")),
        "s_nop": sum(1 for o in ops if o == "s_nop"),
    }


def stats(path):
    """{kernel name: {"meta": ..., "body": ..., "loop": ...}} for the instances of pgx_find_mems_pairs_kernel"""
    md = metadata(path)
    out = {}
    for k, body in I.kernels(path).items():
        if "pgx_find_mems_pairs_kernel" not in k:
            continue
        out[k] = {"meta": md.get(k, {}), "body": count(body), "loop": count(loop_of(body))}
    return out


def is_lce(name):  # the last template argument: ...ILb0ELb1ELb0ELb?ELb1EE...
    m = re.search(r"pgx_find_mems_pairs_kernelILb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)EE", name)
    return bool(m) and m.group(5) == "1"


if __name__ == "__main__":
    for k, s in sorted(stats(sys.argv[1]).items(), key=lambda kv: (not is_lce(kv[0]), kv[0])):
        m = re.search(r"ILb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)EE", k)
        print("<%s>%s" % (",".join(m.groups()) if m else k, "  LCE" if is_lce(k) else ""))
        print("    meta: " + "  ".join("%s %d" % (key, s["meta"].get(key, -1)) for key in META_KEYS))
        for part in ("body", "loop"):
            print("    %s: " % part + "  ".join("%s %d" % kv for kv in s[part].items()))

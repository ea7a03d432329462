"""Instruction and register counts of kernels in two `hipcc -S --offload-arch=gfx950 --cuda-device-only` listings of the
same source file, side by side: shows that a change left a kernel's code alone.  A kernel is named by a substring of its
mangled symbol in each listing (a kernel that became a template changes its symbol: k_predict_rowsEPK -> k_predict_rowsILb0E).

    python tools/isa_compare.py parent.s new.s k_predict_rowsEPK:k_predict_rowsILb0E k_predict_borderEPK:k_predict_borderILb0E
"""
import re, sys


def kernels(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            out[cur] = {"instructions": [], "meta": {}}
            continue
        if cur is None:
            continue
        t = line.strip()
        if t.startswith(".end_amdhsa_kernel"):
            cur = None
            continue
        m = re.match(r"^\.amdhsa_(next_free_vgpr|next_free_sgpr|accum_offset|group_segment_fixed_size|private_segment_fixed_size) (\d+)", t)
        if m:
            out[cur]["meta"][m.group(1)] = int(m.group(2))
        elif t and t[0] not in ";." and not t.endswith(":"):
            out[cur]["instructions"].append(re.sub(r"\s*;.*$", "", t))
    return out


def pick(ks, part):
    hits = [k for k in ks if part in k and ks[k]["meta"]]
    assert len(hits) == 1, (part, hits)
    return ks[hits[0]]


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
same = True
for pair in sys.argv[3:]:
    pa, _, pb = pair.partition(":")
    A, B = pick(a, pa), pick(b, pb or pa)
    strip = lambda ins: [re.sub(r"\.LBB\d+_", ".LBB_", i) for i in ins]
    differing = sum(x != y for x, y in zip(strip(A["instructions"]), strip(B["instructions"])))
    ok = len(A["instructions"]) == len(B["instructions"]) and A["meta"] == B["meta"]
    same = same and ok
    print(f"{pair}: instructions {len(A['instructions'])} / {len(B['instructions'])}, {A['meta']} / {B['meta']}, "
          f"lines that differ beyond label numbers: {differing}  {'EQUAL COUNTS' if ok else 'DIFFERENT'}")
sys.exit(0 if same else 1)

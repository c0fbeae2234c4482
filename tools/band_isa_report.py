"""Resource report of the band kernel's instances from hipcc's -save-temps listing, and the comparison of two builds:

    python tools/band_isa_report.py branch.s [parent.s]

Per kernel whose name contains `render_band` (the 24 one-shot instances and the 24 carry instances) one line out of the code object's metadata
(.vgpr_count, .sgpr_count, the spill counts, scratch and LDS bytes).  With a second listing: the same figures of the kernel of that name there, and
whether the two instruction streams are the same once labels, comments and assembler directives are taken out (branch targets are renumbered in
order of first appearance, so a listing in which every label moved by a constant compares equal)."""
import re
import subprocess
import sys

FIELDS = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def metadata(asm):
    """{kernel name: {field: int}} from the .amdgpu_metadata document at the end of the listing."""
    doc = asm[asm.index(".amdgpu_metadata"):]
    out = {}
    for blk in re.split(r"\n  - \.agpr_count:", doc)[1:]:
        name = re.search(r"\n\s+\.name:\s+(\S+)", blk).group(1)
        out[name] = {f: int(re.search(r"\n\s+%s:\s+(\d+)" % re.escape(f), blk).group(1)) for f in FIELDS}
    return out


def body_of(asm, name):
    a = asm.index("\n" + name + ":") + 1
    return asm[a:asm.index(".Lfunc_end", a)].split("\n")


def stream(asm, name):
    """The kernel's instructions, labels renumbered by first appearance."""
    labels, out = {}, []
    lab = lambda m: labels.setdefault(m.group(0), "L%d" % len(labels))
    for raw in body_of(asm, name)[1:]:
        line = raw.split(";")[0].strip()
        if not line or (line.startswith(".") and not line.endswith(":")):
            continue
        out.append(re.sub(r"\.LBB\d+_\d+", lab, line))
    return out


def short(name):
    dn = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    m = re.search(r"(render_band\w*<[^(]*>)\(", dn)
    return (m.group(1) if m else dn).replace("gmpi::", "")


def main():
    new = open(sys.argv[1]).read()
    old = open(sys.argv[2]).read() if len(sys.argv) > 2 else None
    meta_new, meta_old = metadata(new), metadata(old) if old else {}
    names = sorted(n for n in meta_new if "render_band" in n)
    row = lambda m: " ".join("%5d" % m[f] for f in FIELDS)
    print("%-70s %s" % ("kernel", " ".join(f.lstrip(".").replace("_count", "").replace("_fixed_size", "")[:12] for f in FIELDS)))
    same = differ = 0
    for n in names:
        line = "%-70s %s" % (short(n), row(meta_new[n]))
        if n in meta_old:
            eq = stream(new, n) == stream(old, n)
            same, differ = same + eq, differ + (not eq)
            line += "   | parent %s   stream %s" % (row(meta_old[n]), "identical" if eq else "DIFFERS")
        print(line)
    if old:
        print("instances in both builds: %d, identical instruction streams: %d, different: %d" % (same + differ, same, differ))
    return 0


if __name__ == "__main__":
    sys.exit(main())

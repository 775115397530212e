"""Compare the gfx950 kernels of two builds of libsiren_mri_amd.so, kernel by kernel (a host-side
change reorders the kernels inside the code object, so whole-file hashes say nothing):

    python tools/compare_code_objects.py PARENT.so BRANCH.so [--allow-removed NAME ...] [-o summary.txt]

For every kernel of both: the instruction stream (llvm-objdump -d; addresses and encodings dropped,
and the literal of an s_add_u32 / s_addc_u32 that follows s_getpc_b64 masked — a pc-relative
offset to data outside the kernel) and the resource metadata (VGPR / AGPR / SGPR counts, LDS and
scratch bytes, from the code object's amdhsa.kernels note). Exit status 1 if a kernel differs, is
missing from the branch without being allowed, or is new in the branch.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from extract_code_objects import LLVM, extract  # noqa: E402

META = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels_of(lib, outdir):
    """demangled-free symbol -> (instruction lines, metadata dict) over every code object of lib."""
    out = {}
    for dis in extract(lib, outdir):
        kernels = []
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", dis[:-4] + ".co"], capture_output=True,
                               text=True, check=True).stdout
        for line in notes.splitlines():  # amdhsa.kernels: "  - .key: v" opens an entry, "    .key: v" continues it
            m = re.match(r"^  (- |  )\.(\w+):\s*(.*)$", line)
            if not m:
                continue
            if m.group(1) == "- ":
                kernels.append({})
            kernels[-1][m.group(2)] = m.group(3).strip().strip("'")
        meta = {k["name"]: k for k in kernels}
        name, pc = None, 0
        for line in open(dis):
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:  # a kernel, or a device function that kernels call (no metadata of its own)
                name = m.group(1)
                out[name] = ([], {k: meta.get(name, {}).get(k) for k in META})
                continue
            if name is None or not line.startswith("\t"):
                continue
            ins = line.split("//")[0].strip()
            if pc and re.match(r"^s_addc?_u32 ", ins):
                ins = re.sub(r"(0x[0-9a-f]+|-?\d+)$", "<pcrel>", ins)
                pc -= 1
            else:
                pc = 2 if ins.startswith("s_getpc_b64") else 0
            out[name][0].append(ins)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--allow-removed", nargs="*", default=[], help="substrings of kernels the branch may drop")
    ap.add_argument("-o", "--out")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        par = kernels_of(a.parent, os.path.join(tmp, "parent"))
        br = kernels_of(a.branch, os.path.join(tmp, "branch"))
    removed = sorted(set(par) - set(br))
    added = sorted(set(br) - set(par))
    bad_removed = [k for k in removed if not any(s in k for s in a.allow_removed)]
    code = [k for k in par if k in br and par[k][0] != br[k][0]]
    meta = [k for k in par if k in br and par[k][1] != br[k][1]]
    lines = [f"kernels: parent {len(par)}, branch {len(br)}, in both {len(set(par) & set(br))}",
             f"instructions compared: {sum(len(par[k][0]) for k in par if k in br)}",
             f"removed from the branch ({len(removed)}): {' '.join(removed) or '-'}",
             f"new in the branch ({len(added)}): {' '.join(added) or '-'}",
             f"instruction stream differs ({len(code)}): {' '.join(code) or '-'}",
             f"resource metadata differs ({len(meta)}): {' '.join(meta) or '-'}   [{', '.join(META)}]"]
    ok = not (bad_removed or added or code or meta)
    lines.append("RESULT: " + ("identical per kernel" if ok else "DIFFERENT"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

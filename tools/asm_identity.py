"""Compare the device assembly of two builds of the group translation units, kernel by kernel.

    hipcc --offload-device-only -S ... -o <dir>/<group>.s      (once per build and group, flags of libff_amd/build.py)
    python tools/asm_identity.py <dir_before> <dir_after>

Comments and assembler directives are dropped, the ordinals that count functions or long branches of the whole file inside
local labels (.LBB<fn>_<block>, .Lpost_getpc<k>) are removed, and a function's body is what stands between its label and the next function's label.  Reports, per group, the
functions whose text differs and the ones only one side has; exit code 1 when a function of the first build differs or
is gone.  (DESIGN sections 9 and 10 quote its outcome.)
"""
import os
import re
import sys


def functions(path):
    """{label: [instruction lines]} of every global function / kernel label of an AMDGPU .s file"""
    out, cur = {}, None
    for raw in open(path, errors="replace"):
        line = raw.split(";", 1)[0].rstrip()
        if not line.strip():
            continue
        m = re.match(r"^([A-Za-z_$][\w$.]*):\s*$", line)
        if m and not m.group(1).startswith((".L", "__hip_cuid", "amdhsa")):
            cur = out.setdefault(m.group(1), [])
            continue
        if line.lstrip().startswith(".") and not re.match(r"^\s*\.LBB\S*:", line):
            if line.lstrip().startswith((".amdhsa_kernel", ".section", ".text", ".rodata", ".amdgpu_metadata")):
                cur = None if not line.lstrip().startswith(".text") else cur
            continue   # directive
        if cur is not None:
            # local labels carry the function's ordinal in the file (.LBB<fn>_<block>), which moves when a kernel is added
            # (so does the file-wide ordinal of a long branch's .Lpost_getpc<k> label)
            cur.append(re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", re.sub(r"\.L(BB|JTI|CPI)\d+_", r".L\1_", line.strip())))
    return out


def main(before, after):
    bad = 0
    for name in sorted(os.listdir(before)):
        if not name.endswith(".s") or not os.path.exists(os.path.join(after, name)):
            continue
        a, b = functions(os.path.join(before, name)), functions(os.path.join(after, name))
        differ = sorted(k for k in a if k in b and a[k] != b[k])
        gone = sorted(k for k in a if k not in b)
        new = sorted(k for k in b if k not in a)
        same = sum(1 for k in a if k in b and a[k] == b[k])
        print(f"{name}: {same} functions identical, {len(differ)} differ, {len(gone)} removed, {len(new)} added")
        for k in differ:
            print("   differs:", k)
        for k in gone:
            print("   removed:", k)
        for k in new:
            print("   added:  ", k)
        bad += len(differ) + len(gone)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))

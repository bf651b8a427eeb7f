#!/usr/bin/env python3
"""Development aid: show that two builds of libbgm_hip.so carry the same gfx950 device code, without a GPU.

    python -m bayesgm_amd.csrc.build --force -o A/libbgm_hip.so      (at one commit)
    python -m bayesgm_amd.csrc.build --force -o B/libbgm_hip.so      (at the other)
    python scripts/compare_code_objects.py A B

For every object file (*.o) of the two build directories the gfx950 code object is extracted (llvm-objdump --offloading, into a
temporary directory) and compared per kernel symbol:
  * the kernel descriptors' metadata (llvm-readelf --notes): the set of kernel names, and per kernel .vgpr_count, .sgpr_count,
    .agpr_count, .private_segment_fixed_size, .group_segment_fixed_size, .kernarg_segment_size, .max_flat_workgroup_size;
  * the disassembly (llvm-objdump -d) of every function symbol: mnemonics, operands and encodings, without the addresses.
The order of the kernels inside an object does not matter.  Prints one line per object and a total; exit status 1 on any difference.
It reads the two directories and nothing else.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
FIELDS = (".vgpr_count", ".sgpr_count", ".agpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size", ".kernarg_segment_size",
          ".max_flat_workgroup_size")


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name)] + list(args), check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp):
    """the gfx950 code object inside a host object file (None when it has no device code)"""
    work = os.path.join(tmp, os.path.basename(obj))
    shutil.copy(obj, work)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", work], check=True, capture_output=True, cwd=tmp)
    found = [f for f in os.listdir(tmp) if f.startswith(os.path.basename(work) + ".") and f.endswith("gfx950")]
    return os.path.join(tmp, found[0]) if found else None


def kernel_metadata(co):
    """{kernel name: {field: value}} from the AMDGPU metadata note"""
    kernels, cur = {}, None
    for line in tool("llvm-readelf", "--notes", co).splitlines():
        if line.startswith("  - "):      # a new entry of amdhsa.kernels
            cur = {}
            line = "    " + line[4:]
        m = re.match(r"    (\.\w+):\s+(\S+)$", line)
        if m and cur is not None:
            if m.group(1) == ".name":
                kernels[m.group(2)] = cur
            elif m.group(1) in FIELDS:
                cur[m.group(1)] = m.group(2)
    return kernels


def disassembly(co):
    """{symbol: [instruction text + encoding]}; addresses and the <symbol+offset> notes of branches are dropped"""
    funcs, cur = {}, None
    for line in tool("llvm-objdump", "-d", co).splitlines():
        m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
        elif cur is not None and "//" in line:
            text, note = line.split("//", 1)
            enc = re.sub(r"<[^>]*>", "", note.split(":", 1)[1]).split()
            cur.append(text.strip() + " | " + " ".join(enc))
    return funcs


def compare(a, b, tmp):
    """(kernels compared, list of differences) of one object file present in both directories"""
    ta, tb = os.path.join(tmp, "a"), os.path.join(tmp, "b")
    os.makedirs(ta), os.makedirs(tb)
    ca, cb = code_object(a, ta), code_object(b, tb)
    if ca is None or cb is None:
        return 0, ([] if ca is cb else ["device code in one build only"])
    diffs = []
    ma, mb = kernel_metadata(ca), kernel_metadata(cb)
    for k in sorted(set(ma) ^ set(mb)):
        diffs.append("kernel in one build only: " + k)
    for k in sorted(set(ma) & set(mb)):
        for f in FIELDS:
            if ma[k].get(f) != mb[k].get(f):
                diffs.append("%s: %s %s -> %s" % (k, f, ma[k].get(f), mb[k].get(f)))
    da, db = disassembly(ca), disassembly(cb)
    for k in sorted(set(da) ^ set(db)):
        diffs.append("function in one build only: " + k)
    for k in sorted(set(da) & set(db)):
        if da[k] != db[k]:
            at = next((i for i, (x, y) in enumerate(zip(da[k], db[k])) if x != y), min(len(da[k]), len(db[k])))
            diffs.append("%s: instructions differ (%d vs %d, first at #%d)" % (k, len(da[k]), len(db[k]), at))
    return len(set(ma) & set(mb)), diffs


def main(dir_a, dir_b):
    objs_a = {f for f in os.listdir(dir_a) if f.endswith(".o")}
    objs_b = {f for f in os.listdir(dir_b) if f.endswith(".o")}
    total_k = total_d = 0
    for f in sorted(objs_a ^ objs_b):
        print("%s: in one build only" % f)
        total_d += 1
    for f in sorted(objs_a & objs_b):
        with tempfile.TemporaryDirectory() as tmp:
            n, diffs = compare(os.path.join(dir_a, f), os.path.join(dir_b, f), tmp)
        print("%s: %d kernels compared, %d differences" % (f, n, len(diffs)))
        for d in diffs:
            print("    " + d)
        total_k += n
        total_d += len(diffs)
    print("total: %d objects, %d kernels compared, %d differences" % (len(objs_a & objs_b), total_k, total_d))
    return 1 if total_d else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))

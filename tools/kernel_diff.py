"""Compare the gfx950 kernels of two builds, kernel by kernel.  CPU only.

    python tools/kernel_diff.py LEFT RIGHT [--all]

LEFT and RIGHT are two object files or two directories of them (matched by file name): the objects riser_amd/build.py leaves in
csrc/build*/ or the output of `hipcc <FLAGS> --cuda-device-only -c`.  The gfx950 code object is taken out of each (a host object
carries it as an offload bundle in .hip_fatbin, a device-only compile is the bundle or the code object itself) and per kernel symbol
three things are compared:
  * hash   sha256[:16] over the instruction encodings of `llvm-objdump -d`, in order; the s_nop / s_code_end padding behind a kernel
           is not counted (bundles are not byte-equal even for an untouched source compiled twice; the encodings are)
  * meta   `llvm-readelf --notes`: VGPRs, AGPRs, SGPRs, fixed LDS bytes, scratch bytes, SGPR / VGPR spill counts
  * counts instructions of the classes v_mfma*, buffer_load*, buffer_store*, ds_read*, ds_write*, s_barrier, v_permlane*
A line per kernel that differs (--all: per kernel), then per file and in total: equal, changed, only-left, only-right.  Of a changed
kernel the line says what moved: `hash` alone is a different instruction stream with the same resources and the same class counts.
Nothing else of the assembly is looked at.  Exit status 0 if every kernel is equal, 1 otherwise.
"""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
META = [("vgpr", ".vgpr_count"), ("agpr", ".agpr_count"), ("sgpr", ".sgpr_count"), ("lds", ".group_segment_fixed_size"),
        ("scratch", ".private_segment_fixed_size"), ("sgpr_spill", ".sgpr_spill_count"), ("vgpr_spill", ".vgpr_spill_count")]
CLASSES = ["v_mfma", "buffer_load", "buffer_store", "ds_read", "ds_write", "s_barrier", "v_permlane"]
PADDING = ("s_nop", "s_code_end")


def llvm(tool):
    for d in (os.environ.get("LLVM_BIN"), "/opt/rocm/llvm/bin", "/opt/rocm/lib/llvm/bin"):
        if d and os.path.exists(os.path.join(d, tool)):
            return os.path.join(d, tool)
    p = shutil.which(tool)
    if not p:
        sys.exit("kernel_diff: %s not found (set LLVM_BIN)" % tool)
    return p


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(path, tmp):
    """the gfx950 ELF inside `path`"""
    with open(path, "rb") as f:
        head = f.read(24)
    bundle = path
    if head[:4] == b"\x7fELF":
        if head[18:20] == (224).to_bytes(2, "little"):                # EM_AMDGPU: already the code object
            return path
        bundle = os.path.join(tmp, "fatbin")
        run(llvm("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + bundle, path)
    out = os.path.join(tmp, "co")
    run(llvm("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + bundle, "--output=" + out)
    return out


def kernels_of(path):
    """{symbol: {"hash", "meta", "counts"}} of one object file"""
    with tempfile.TemporaryDirectory() as tmp:
        co = code_object(path, tmp)
        notes = run(llvm("llvm-readelf"), "--notes", co)
        dis = run(llvm("llvm-objdump"), "-d", co)
    meta, cur = {}, None
    for line in notes.splitlines():
        m = re.match(r"^  (- | {2})(\.\w+):\s*(\S+)\s*$", line)           # a field of a kernel record (not of its .args)
        if line.startswith("  - "):
            cur = {}
        if m and cur is not None:
            cur[m.group(2)] = m.group(3)
            if m.group(2) == ".name":
                meta[m.group(3)] = cur
    out, body = {}, {}
    name = None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1)
            body[name] = []
            continue
        m = re.match(r"^\s+(\S+)\b.*//\s*[0-9A-F]+:((?: [0-9A-F]{8})+)\s*$", line)
        if m and name is not None:
            body[name].append((m.group(1), m.group(2).strip()))
    for name, ins in body.items():
        if name not in meta:                                                  # a device function, not a kernel
            continue
        while ins and ins[-1][0].startswith(PADDING):
            ins.pop()
        h = hashlib.sha256()
        for _, enc in ins:
            h.update(enc.encode())
        out[name] = {"hash": h.hexdigest()[:16],
                     "meta": {k: int(meta[name].get(f, -1)) for k, f in META},
                     "counts": {c: sum(1 for mn, _ in ins if mn.startswith(c)) for c in CLASSES}}
    for name in meta:
        if name not in out:
            sys.exit("kernel_diff: %s: kernel %s has metadata but no code" % (path, name))
    return out


def fmt(k):
    return "%s  %s  %s" % (k["hash"], " ".join("%s=%d" % kv for kv in k["meta"].items()), " ".join("%s=%d" % kv for kv in k["counts"].items()))


def compare(label, left, right, show_all):
    tally = {"equal": 0, "changed": 0, "only-left": 0, "only-right": 0}
    for name in sorted(set(left) | set(right)):
        if name not in right or name not in left:
            side = "only-left" if name in left else "only-right"
            tally[side] += 1
            print("%-10s %s\n           %s" % (side, name, fmt(left.get(name) or right[name])))
            continue
        a, b = left[name], right[name]
        what = [k for k in ("hash",) if a[k] != b[k]]
        what += ["%s %d->%d" % (k, a["meta"][k], b["meta"][k]) for k, _ in META if a["meta"][k] != b["meta"][k]]
        what += ["%s %d->%d" % (c, a["counts"][c], b["counts"][c]) for c in CLASSES if a["counts"][c] != b["counts"][c]]
        tally["changed" if what else "equal"] += 1
        if what:
            print("changed    %s\n           %s\n           left  %s\n           right %s" % (name, ", ".join(what), fmt(a), fmt(b)))
        elif show_all:
            print("equal      %s\n           %s" % (name, fmt(a)))
    print("%-28s %s" % (label, "  ".join("%s %d" % kv for kv in tally.items())))
    return tally


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) != 2:
        sys.exit(__doc__)
    show_all = "--all" in sys.argv
    l, r = args
    if os.path.isdir(l) != os.path.isdir(r):
        sys.exit("kernel_diff: two files or two directories")
    if os.path.isdir(l):
        names = lambda d: {f for f in os.listdir(d) if f.endswith((".o", ".co", ".hsaco"))}
        pairs = [(f, os.path.join(l, f) if f in names(l) else None, os.path.join(r, f) if f in names(r) else None)
                 for f in sorted(names(l) | names(r))]
    else:
        pairs = [(os.path.basename(l), l, r)]
    total = {"equal": 0, "changed": 0, "only-left": 0, "only-right": 0}
    for label, a, b in pairs:
        t = compare(label, kernels_of(a) if a else {}, kernels_of(b) if b else {}, show_all)
        for k in total:
            total[k] += t[k]
    print("%-28s %s" % ("TOTAL", "  ".join("%s %d" % kv for kv in total.items())))
    sys.exit(0 if total["equal"] == sum(total.values()) else 1)


if __name__ == "__main__":
    main()

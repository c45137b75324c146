#!/usr/bin/env python3
"""Are the gfx950 code objects of two builds the same bytes?  (No GPU needed.)

usage: tools/code_object_diff.py OLD_OBJ_DIR NEW_OBJ_DIR     (two copies of black-hole-renderer_amd/lib/obj)

Every *.o of either directory that carries a gfx950 code object is unbundled with llvm-objdump --offloading (as
tools/kernel_resources.sh does) and three things are compared: the raw bytes of .text, the raw bytes of .rodata, and the text
of llvm-readelf --notes (kernel names, registers, LDS, argument layouts).  One line per object: name, .text size, kernel
count, `same` or `DIFFERENT`.  Exit status 1 on any difference or if an object is on one side only."""
import os
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def tool(name):
    return os.path.join(LLVM, name)


def code_object(obj, work):
    """Unbundle obj's gfx950 code object into `work`; its path, or None if obj carries none."""
    os.makedirs(work)
    base = os.path.basename(obj)
    shutil.copy(obj, os.path.join(work, base))
    subprocess.run([tool("llvm-objdump"), "--offloading", base], cwd=work, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    found = sorted(f for f in os.listdir(work) if f.startswith(base + ".") and f.endswith("gfx950"))
    return os.path.join(work, found[0]) if found else None


def section(co, name):
    out = co + name + ".bin"
    subprocess.check_call([tool("llvm-objcopy"), "-O", "binary", "--only-section=" + name, co, out])
    with open(out, "rb") as f:
        return f.read()


def describe(obj, work):
    co = code_object(obj, work)
    if co is None:
        return None
    notes = subprocess.check_output([tool("llvm-readelf"), "--notes", co], text=True)
    kernels = sum(1 for line in notes.splitlines() if line.strip().startswith(".symbol:"))
    return {"text": section(co, ".text"), "rodata": section(co, ".rodata"), "notes": notes, "kernels": kernels}


def main(argv):
    if len(argv) != 3:
        sys.stderr.write(__doc__)
        return 2
    old_dir, new_dir = argv[1], argv[2]
    objs = lambda d: {f for f in os.listdir(d) if f.endswith(".o")}
    old, new = objs(old_dir), objs(new_dir)
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for name in sorted(old | new):
            a = describe(os.path.join(old_dir, name), os.path.join(tmp, "old", name)) if name in old else None
            b = describe(os.path.join(new_dir, name), os.path.join(tmp, "new", name)) if name in new else None
            if a is None and b is None:
                if name in old and name in new:
                    continue   # host code only, on both sides
                bad += 1
                print(f"{name:24s} {'-':>10s} {'-':>3s}  only in {'OLD' if name in old else 'NEW'}")
                continue
            if a is None or b is None:
                bad += 1
                have = a or b
                side = "OLD" if b is None else "NEW"
                print(f"{name:24s} {len(have['text']):10d} {have['kernels']:3d}  DIFFERENT (code object only in {side})")
                continue
            diffs = [k for k in ("text", "rodata", "notes") if a[k] != b[k]]
            if a["kernels"] != b["kernels"]:
                diffs.append(f"kernels {a['kernels']} -> {b['kernels']}")
            bad += bool(diffs)
            verdict = "same" if not diffs else "DIFFERENT (" + ", ".join(diffs) + ")"
            print(f"{name:24s} {len(b['text']):10d} {b['kernels']:3d}  {verdict}")
    print(f"{'all the same' if not bad else str(bad) + ' object(s) differ'}: .text, .rodata and notes of every gfx950 code object")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

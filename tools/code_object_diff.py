#!/usr/bin/env python3
"""Are the gfx950 code objects of two builds the same bytes?  (No GPU needed.)

usage: tools/code_object_diff.py OLD_OBJ_DIR NEW_OBJ_DIR     (two copies of black-hole-renderer_amd/lib/obj)

Every *.o of either directory that carries a gfx950 code object is unbundled with llvm-objdump --offloading (as
tools/kernel_resources.sh does) and three things are compared: the raw bytes of .text, the raw bytes of .rodata, and the text
of llvm-readelf --notes (kernel names, registers, LDS, argument layouts).  One line per object: name, .text size, kernel
count, `same` or `DIFFERENT`.  Exit status 1 on any difference or if an object is on one side only.

Under an object that differs, two lines per kernel symbol of either side (paired by name): VGPRs, SGPRs, private segment and
group segment bytes from the notes and the instruction count `n` from llvm-objdump -d, each as `old` or `old -> new`, and
whether the instruction text is the same.  Instruction text is mnemonic and operands only: addresses, encodings and the
branch-target labels (symbol + offset, which move with the kernel's place in .text) are dropped; a branch keeps its relative
offset.  A kernel on one side only is listed as such, with the other side's one-sided kernels of the same text, if any.

Behind the objects, the kernels of the code objects that are on one side only (a source split or renamed): each OLD one with its
resources and the NEW ones of the same instruction text and resources -- where it moved to -- or `no twin`."""
import difflib
import os
import re
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
    return {"text": section(co, ".text"), "rodata": section(co, ".rodata"), "notes": notes, "kernels": kernels, "co": co}


NOTE_FIELDS = (("vgpr", "vgpr_count"), ("sgpr", "sgpr_count"), ("private", "private_segment_fixed_size"), ("lds", "group_segment_fixed_size"))


def per_kernel(d):
    """{kernel symbol: resources from the notes + "insts": its instruction text, a list}"""
    col = lambda key: re.findall(r"^\s*-?\s*\." + key + r":\s*(\S+)", d["notes"], re.M)   # once per kernel, in the kernels' order
    names = [s[:-3] if s.endswith(".kd") else s for s in col("symbol")]
    out = {n: {"insts": []} for n in names}
    for short, key in NOTE_FIELDS:
        for n, v in zip(names, col(key)):
            out[n][short] = int(v)
    cur = None
    for line in subprocess.check_output([tool("llvm-objdump"), "-d", d["co"]], text=True).splitlines():
        label = re.match(r"^[0-9a-fA-F]+ <(.+)>:$", line)
        if label:
            cur = out.get(label.group(1))
        elif cur is not None and line.startswith(("\t", " ")) and line.strip():
            cur["insts"].append(" ".join(line.split("//")[0].split()))
    for k in out.values():   # the padding behind a kernel's last instruction is not its code
        while k["insts"] and k["insts"][-1].split()[0] in ("s_code_end", "s_nop", "..."):   # "...": objdump's mark for a run of zero bytes
            k["insts"].pop()
    return out


def kernel_breakdown(a, b):
    ka, kb = per_kernel(a), per_kernel(b)
    for k in list(ka.values()) + list(kb.values()):
        k["n"] = len(k["insts"])
    keys = ("vgpr", "sgpr", "private", "lds", "n")
    for sym in sorted(set(ka) | set(kb)):
        if sym in ka and sym in kb:
            x, y = ka[sym], kb[sym]
            cols = " ".join(f"{k} {x[k]}" + ("" if x[k] == y[k] else f" -> {y[k]}") for k in keys)
            if x["insts"] == y["insts"]:
                text = "text same"
            else:   # how many instructions of either side are outside a longest common run of lines
                kept = sum(m.size for m in difflib.SequenceMatcher(None, x["insts"], y["insts"], autojunk=False).get_matching_blocks())
                text = f"text DIFFERENT ({x['n'] - kept} old, {y['n'] - kept} new instructions unmatched)"
        else:       # on one side only; a renamed kernel shows as a kernel of the other side only with the same text
            here, there, side, other = (ka, kb, "OLD", "NEW") if sym in ka else (kb, ka, "NEW", "OLD")
            x = here[sym]
            cols = " ".join(f"{k} {x[k]}" for k in keys)
            twins = [t for t in sorted(there) if t not in here and there[t]["insts"] == x["insts"]]
            text = f"only in {side}" + "".join(f"; text same as {other}'s {t}" for t in twins)
        print(f"    {sym}\n        {cols}  {text}")


def moved_kernels(old_only, new_only):
    """old_only, new_only: {object name: describe()} of the code objects on one side only."""
    keys = ("vgpr", "sgpr", "private", "lds")
    new = [(name, sym, k) for name, d in sorted(new_only.items()) for sym, k in sorted(per_kernel(d).items())]
    print("kernels of the code objects on one side only:")
    for name, d in sorted(old_only.items()):
        for sym, x in sorted(per_kernel(d).items()):
            cols = " ".join(f"{k} {x[k]}" for k in keys) + f" n {len(x['insts'])}"
            twins = [f"{n}: {s}" for n, s, y in new if y["insts"] == x["insts"] and all(y[k] == x[k] for k in keys)]
            print(f"    OLD {name}: {sym}\n        {cols}  " + ("; ".join("same text and resources as NEW " + t for t in twins) or "no twin in NEW"))


def main(argv):
    if len(argv) != 3:
        sys.stderr.write(__doc__)
        return 2
    old_dir, new_dir = argv[1], argv[2]
    objs = lambda d: {f for f in os.listdir(d) if f.endswith(".o")}
    old, new = objs(old_dir), objs(new_dir)
    bad = 0
    old_only, new_only = {}, {}
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
                (old_only if b is None else new_only)[name] = have
                print(f"{name:24s} {len(have['text']):10d} {have['kernels']:3d}  DIFFERENT (code object only in {side})")
                continue
            diffs = [k for k in ("text", "rodata", "notes") if a[k] != b[k]]
            if a["kernels"] != b["kernels"]:
                diffs.append(f"kernels {a['kernels']} -> {b['kernels']}")
            bad += bool(diffs)
            verdict = "same" if not diffs else "DIFFERENT (" + ", ".join(diffs) + ")"
            print(f"{name:24s} {len(b['text']):10d} {b['kernels']:3d}  {verdict}")
            if diffs:
                kernel_breakdown(a, b)
        if old_only and new_only:
            moved_kernels(old_only, new_only)
    print(f"{'all the same' if not bad else str(bad) + ' object(s) differ'}: .text, .rodata and notes of every gfx950 code object")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

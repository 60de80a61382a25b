#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libdlp.so, function by function.

    tools/kernel_diff.py OLD.so NEW.so

For a change that only moves kernels between translation units (or touches host code), the
device code must not change.  Both libraries' bundled code objects are extracted and every
function symbol is compared:

  * its instruction text, without the address / encoding comments, and with the literals of the
    instructions that follow an s_getpc_b64 masked: those are pc-relative distances to globals,
    which move with the layout of the code object (branch operands are relative already);
  * for kernels, the descriptor: the resource fields of the metadata note and the 64-byte kernel
    descriptor (<kernel>.kd) with its code-entry offset masked.

Prints one line per difference and a summary; exit status 1 when anything differs."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
NOTE_FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size",
               ".private_segment_fixed_size", ".wavefront_size", ".kernarg_segment_size",
               ".max_flat_workgroup_size", ".uses_dynamic_stack")
PCREL_WINDOW = 3   # instructions after s_getpc_b64 whose literals are layout-dependent


def run(d, tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], cwd=d, check=True, capture_output=True,
                          text=True).stdout


def functions(text):
    """{symbol: [instruction lines]} of a disassembly, pc-relative literals masked."""
    funcs, cur, mask = {}, None, 0
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line.strip())
        if m:
            cur, mask = funcs.setdefault(m.group(1), []), 0
            continue
        line = line.split("//")[0].strip()
        if cur is None or not line or line.endswith(":") or line == "...":   # ("...": elided zero padding)
            continue
        if mask:
            line, mask = re.sub(r"\b0x[0-9a-f]+\b", "<pcrel>", line), mask - 1
        if line.startswith("s_getpc_b64"):
            mask = PCREL_WINDOW
        cur.append(line)
    return funcs


def note_descriptors(notes):
    """{kernel: {field: value}} from `llvm-readelf --notes` (the amdhsa.kernels list)."""
    out, cur, item = {}, None, None
    for line in notes.splitlines():
        if line.strip() == "amdhsa.kernels:":
            item = ""
            continue
        if item is None:
            continue
        ind = len(line) - len(line.lstrip())
        body = line.strip()
        if item == "" and body.startswith("- "):
            item = " " * ind + "- "
        if item and line.startswith(item):          # a new kernel entry
            cur = {}
            body = body[2:]
            ind += 2
        elif item and ind <= len(item) - 2 and body:  # the list is over
            item, cur = None, None
            continue
        if cur is None or ind != len(item):
            continue
        key, _, val = body.partition(":")
        if key == ".name":
            out[val.strip()] = cur
        elif key in NOTE_FIELDS:
            cur[key] = val.strip()
    return out


def kd_bytes(d, f):
    """{kernel: 64-byte descriptor, code-entry offset (bytes 16-23) zeroed}."""
    secs = []
    for line in run(d, "llvm-readelf", "-S", "--wide", f).splitlines():
        m = re.match(r"\s*\[\s*\d+\]\s+\S+\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            secs.append(tuple(int(x, 16) for x in m.groups()))
    blob = open(os.path.join(d, f), "rb").read()
    out = {}
    for line in run(d, "llvm-readelf", "-s", "--wide", f).splitlines():
        p = line.split()
        if len(p) >= 8 and p[7].endswith(".kd"):
            addr = int(p[1], 16)
            off = next(o + addr - a for a, o, n in secs if a <= addr < a + n)
            kd = bytearray(blob[off:off + 64])
            kd[16:24] = bytes(8)
            out[p[7][:-3]] = bytes(kd).hex()
    return out


def load(so):
    """(functions, descriptors, duplicates) of every gfx950 code object bundled in `so`."""
    funcs, descs, dups = {}, {}, []
    with tempfile.TemporaryDirectory() as d:
        lib = os.path.join(d, "lib.so")
        with open(so, "rb") as src, open(lib, "wb") as dst:
            dst.write(src.read())
        run(d, "llvm-objdump", "--offloading", "lib.so")
        for f in sorted(os.listdir(d)):
            if "amdgcn" not in f or "gfx950" not in f:
                continue
            fs = functions(run(d, "llvm-objdump", "-d", "--mcpu=gfx950", f))
            dups += [n for n in fs if n in funcs]
            funcs.update(fs)
            notes = note_descriptors(run(d, "llvm-readelf", "--notes", f))
            for k, kd in kd_bytes(d, f).items():
                dups += [k + ".kd"] if k in descs else []
                descs[k] = dict(notes.get(k, {}), kd=kd)
    return funcs, descs, dups


def main(old, new):
    fo, do, dupo = load(old)
    fn, dn, dupn = load(new)
    bad = 0
    for tag, dup in (("OLD", dupo), ("NEW", dupn)):
        for n in dup:
            print(f"DUPLICATE in {tag}: {n}")
            bad += 1
    for n in sorted(set(fo) - set(fn)):
        print(f"MISSING in NEW: {n}")
        bad += 1
    for n in sorted(set(fn) - set(fo)):
        print(f"ADDED in NEW: {n}")
        bad += 1
    for n in sorted(set(do) ^ set(dn)):
        print(f"KERNEL SET differs: {n}")
        bad += 1
    for n in sorted(set(fo) & set(fn)):
        if fo[n] != fn[n]:
            k = next((i for i, (a, b) in enumerate(zip(fo[n], fn[n])) if a != b), min(len(fo[n]), len(fn[n])))
            print(f"INSTRUCTIONS differ: {n}: {len(fo[n])} vs {len(fn[n])} instructions, first at #{k}")
            bad += 1
    for n in sorted(set(do) & set(dn)):
        if do[n] != dn[n]:
            print(f"DESCRIPTOR differs: {n}:\n  old {do[n]}\n  new {dn[n]}")
            bad += 1
    ins = sum(len(v) for v in fn.values())
    print(f"old: {len(fo)} functions, {len(do)} kernels; new: {len(fn)} functions, {len(dn)} kernels, "
          f"{ins} instructions; {bad} differences")
    if not bad:
        print("IDENTICAL: same kernel names, instruction text and descriptors")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))

"""Per-kernel digest of the gfx950 machine code in object files or a built library (CPU only):

    python tools/kernel_isa.py adaptigraph_amd/csrc/*.o                 one line per kernel
    python tools/kernel_isa.py --a old/*.o --b new/*.o                  compare two builds by kernel name; exit 1 on any difference
    python tools/kernel_isa.py --a old/lib.so --b adaptigraph_amd/libadaptigraph_hip.so

A line holds the sha256 (16 hex digits) of the kernel's instruction stream — `llvm-objdump -d` text without addresses, encodings and the padding
behind the last instruction — its instruction count and the resource figures of the code-object metadata (`llvm-readelf --notes`): architectural,
accumulation and scalar registers, LDS bytes, scratch bytes, spilled vector / scalar registers.  Two builds of unchanged kernels print the same lines
whatever the kernels' translation units, their order or their neighbours are; a change that claims "no kernel change" can show that here.
"""
import argparse
import glob
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
FIGURES = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")
PADDING = ("...", "s_nop 0", "s_code_end")


def run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True, text=True).stdout


def kernels(paths):
    """{kernel name: (digest, instruction count, figures)} over the gfx950 code objects bundled in `paths`."""
    found = {}
    with tempfile.TemporaryDirectory() as tmp:
        for n, path in enumerate(paths):
            local = os.path.join(tmp, f"{n}_{os.path.basename(path)}")      # (the bundles are extracted next to their input)
            shutil.copy(path, local)
            run("llvm-objdump", "--offloading", local)
        for co in sorted(glob.glob(os.path.join(tmp, "*gfx950*"))):
            figures = {}
            for block in re.split(r"\n  - (?=\.)", run("llvm-readelf", "--notes", co)):
                name = re.search(r"^\s*\.name:\s+(\S+)", block, re.M)
                if name and ".vgpr_count" in block:
                    figures[name.group(1)] = tuple(int(re.search(rf"\.{f}:\s+(\d+)", block).group(1)) for f in FIGURES)
            stream, cur = {}, None
            for line in run("llvm-objdump", "-d", co).splitlines():
                head = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if head:
                    cur = stream.setdefault(head.group(1), [])
                elif cur is not None and line.strip():
                    cur.append(line.split("//")[0].strip())
            for name, fig in figures.items():
                ins = stream[name]
                while ins and ins[-1] in PADDING:
                    ins.pop()
                if name in found:
                    sys.exit(f"kernel defined twice: {name}")
                found[name] = (hashlib.sha256("\n".join(ins).encode()).hexdigest()[:16], len(ins), fig)
    return found


def show(name, k):
    return f"{k[0]} {k[1]:6d} ins  v{k[2][0]} a{k[2][1]} s{k[2][2]} lds {k[2][3]} scratch {k[2][4]} spill {k[2][5]}/{k[2][6]}  {name}"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("files", nargs="*", help="object files / libraries to list")
    ap.add_argument("--a", nargs="+", default=[], help="first build of a comparison")
    ap.add_argument("--b", nargs="+", default=[], help="second build of a comparison")
    args = ap.parse_args()
    if bool(args.a) != bool(args.b) or bool(args.a) == bool(args.files):
        ap.error("give either files to list or both --a and --b")
    a = kernels(args.files or args.a)
    names = sorted(a)
    if args.files:
        for n in names:
            print(show(n, a[n]))
        print(f"{len(a)} kernels")
        return 0
    b = kernels(args.b)
    differ = [n for n in names if n in b and a[n] != b[n]]
    missing, new = [n for n in names if n not in b], sorted(n for n in b if n not in a)
    for n in differ:
        print(f"DIFFERS\n  a: {show(n, a[n])}\n  b: {show(n, b[n])}")
    for n in missing:
        print(f"MISSING in b: {show(n, a[n])}")
    for n in new:
        print(f"NEW in b:     {show(n, b[n])}")
    print(f"{len(a)} kernels in a, {len(b)} in b: {len(a) - len(differ) - len(missing)} identical, {len(differ)} differ, {len(missing)} missing, {len(new)} new")
    return 1 if differ or missing or new else 0


if __name__ == "__main__":
    sys.exit(main())

"""Are the GPU kernels of two builds the same, instruction for instruction?  (llvm-objdump only; runs without a GPU.)

    python tools/kernel_identity.py OLD NEW [--md OUT.md] [--show N]

OLD and NEW are each a built library (libplmc_hip.so), an object file, or a directory of them (csrc/build).  Every gfx950 code object
is extracted (llvm-objdump --offloading) and disassembled; of each line the address, the encoding and the `<symbol+offset>` note of a
branch are dropped, and the instruction text that is left is compared function by function, under the mangled name.  The order of the
kernels in a code object and the file a kernel was instantiated from do not matter.  A host-only refactor must report the same set of
names and no kernel that differs.  Exit status 1 if anything differs.

The comparison is of text: no instruction is looked for or judged."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

OBJDUMP = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/lib/llvm/bin/llvm-objdump")


def _inputs(path):
    if os.path.isdir(path):
        return sorted(os.path.join(path, f) for f in os.listdir(path) if f.endswith((".so", ".o")))
    return [path]


def disassemble(path):
    """{(mangled name, occurrence): [instruction text, ...]} and the set of kernel names (those with a descriptor `<name>.kd`)."""
    funcs, kernels, seen = {}, set(), {}
    tmp = tempfile.mkdtemp(prefix="plmc_kid_")
    try:
        for i, src in enumerate(_inputs(path)):
            sub = os.path.join(tmp, str(i))
            os.mkdir(sub)
            subprocess.run([OBJDUMP, "--offloading", shutil.copy(src, sub)], cwd=sub, capture_output=True, check=True)
            for f in sorted(os.listdir(sub)):
                if "amdgcn" not in f:
                    continue
                co = os.path.join(sub, f)
                syms = subprocess.run([OBJDUMP, "-t", co], capture_output=True, text=True, check=True).stdout
                kernels.update(m.group(1) for m in re.finditer(r"\s(\S+)\.kd$", syms, re.M))
                cur = None
                for raw in subprocess.run([OBJDUMP, "-d", co], capture_output=True, text=True, check=True).stdout.splitlines():
                    m = re.match(r"^[0-9a-f]+ <(.+)>:", raw)
                    if m:
                        k = seen[m.group(1)] = seen.get(m.group(1), -1) + 1
                        cur = funcs.setdefault((m.group(1), k), [])
                        continue
                    ins = raw.split("//")[0].strip()
                    if cur is not None and ins and not ins.endswith(":") and ins != "...":   # (`...`: zero padding behind a function, elided)
                        cur.append(ins)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return funcs, kernels


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    pretty = out.stdout.splitlines() if out.returncode == 0 else list(names)
    return [re.sub(r"^void plmc::", "", p[:p.index(">(") + 1] if ">(" in p else p.split("(")[0]) for p in pretty]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--md", default=None, help="also write the report to this file")
    ap.add_argument("--show", type=int, default=20, help="how many names of each list to print")
    a = ap.parse_args()
    (fo, ko), (fn, kn) = disassemble(a.old), disassemble(a.new)
    only_old, only_new = sorted(set(fo) - set(fn)), sorted(set(fn) - set(fo))
    both = sorted(set(fo) & set(fn))
    differ = [k for k in both if fo[k] != fn[k]]
    lines = ["old: %s" % a.old, "new: %s" % a.new, "",
             "functions (kernels among them): old %d (%d), new %d (%d)" % (len(fo), len(ko), len(fn), len(kn)),
             "names only in old: %d" % len(only_old), "names only in new: %d" % len(only_new),
             "instruction-identical: %d" % (len(both) - len(differ)), "different: %d" % len(differ),
             "instructions compared: %d" % sum(len(fo[k]) for k in both)]
    for title, keys in (("only in old", only_old), ("only in new", only_new), ("different", differ)):
        if keys:
            lines += ["", "%s:" % title]
            for k, p in list(zip(keys, demangle([k[0] for k in keys])))[:a.show]:
                note = ""
                if title == "different":
                    first = next((i for i, (x, y) in enumerate(zip(fo[k], fn[k])) if x != y), min(len(fo[k]), len(fn[k])))
                    note = "  (%d / %d instructions, first difference at %d)" % (len(fo[k]), len(fn[k]), first)
                lines.append("  %s%s" % (p, note))
            if len(keys) > a.show:
                lines.append("  ... and %d more" % (len(keys) - a.show))
    text = "\n".join(lines) + "\n"
    if a.md:
        with open(a.md, "w") as fh:
            fh.write(text)
    sys.stdout.write(text)
    return 1 if only_old or only_new or differ else 0


if __name__ == "__main__":
    sys.exit(main())

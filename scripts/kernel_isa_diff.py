#!/usr/bin/env python3
"""Compare the gfx950 machine code of the kernels of two source trees, kernel by kernel.

    python scripts/kernel_isa_diff.py <tree A> <tree B> <file under mimo_unet_amd/csrc> [...]
    python scripts/kernel_isa_diff.py ../parent . optim.hip evidential_eval.hip optim_clip/grad_clip.hip
    python scripts/kernel_isa_diff.py <tree A> <tree B> <files of tree A> -- <files of tree B>

Each file is compiled to device assembly in both trees with the Makefile's flags (no GPU needed).  Kernels are matched by
their unqualified name, so a kernel may move between files and namespaces.  Of each kernel the instruction stream and the
.amdhsa_* descriptor lines are compared after removing what only file position causes: comments, the numbers of the
.LBB<n>_<m> / .Ltmp<n> labels (renumbered in order of appearance) and the spelling of the kernel's own symbol.
Prints one line per kernel — identical or not, with VGPRs / SGPRs / LDS bytes / scratch bytes of both sides — and a
unified diff of every kernel that differs.  Exit status 1 when a kernel differs or exists on one side only.
"""
import difflib
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "--cuda-device-only", "-S"]
RESOURCES = (("vgpr", "NumVgprs"), ("sgpr", "TotalNumSgprs"), ("lds", "LDSByteSize"), ("scratch", "ScratchSize"))


def demangle(symbols):
    tool = os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "llvm", "bin", "llvm-cxxfilt")
    if not os.path.exists(tool):
        tool = "c++filt"
    out = subprocess.run([tool], input="\n".join(symbols), capture_output=True, text=True, check=True).stdout
    return dict(zip(symbols, out.splitlines()))


def unqualified(demangled):
    """'void mimo::a::k<1, true>(float*, ...)' -> 'k<1, true>'"""
    text = demangled.replace("(anonymous namespace)", "anon")
    depth, start = 0, 0
    for i, ch in enumerate(text):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif depth == 0 and ch == "(":  # the parameter list
            return text[start:i]
        elif depth == 0 and ch in " :":  # behind the return type of a template instance, behind a qualifier
            start = i + 1
    return text[start:]


def kernels_of(asm):
    """{mangled symbol: (normalised lines, resources)} of one device assembly text"""
    lines = asm.splitlines()
    found = {}
    for sym in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M):
        first = lines.index(sym + ":") if sym + ":" in lines else next(
            i for i, l in enumerate(lines) if l.startswith(sym + ":"))
        last = next(i for i in range(first, len(lines)) if lines[i].strip().startswith(".end_amdhsa_kernel"))
        tmp = {}
        body = []
        for l in lines[first:last + 1]:
            l = l.split(";", 1)[0].rstrip()
            if not l.strip():
                continue
            l = l.replace(sym, "<kernel>")
            # labels are numbered in the order in which the kernel's text first names them
            l = re.sub(r"\.(LBB\d+_|Ltmp)\d+", lambda m: tmp.setdefault(m.group(0), ".L#%d" % len(tmp)), l)
            l = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", l)
            body.append(l)
        res = {}
        for l in lines[last:last + 80]:
            for key, word in RESOURCES:
                m = re.match(r";\s*%s:\s*(\d+)" % word, l.strip())
                if m and key not in res:
                    res[key] = int(m.group(1))
        found[sym] = (body, res)
    return found


def compile_tree(tree, files, tmpdir, tag):
    out = {}
    for f in files:
        s = os.path.join(tmpdir, "%s_%s.s" % (tag, f.replace("/", "_")))
        subprocess.run([HIPCC] + FLAGS + [os.path.join(tree, "mimo_unet_amd", "csrc", f), "-o", s], check=True)
        with open(s) as fh:
            ks = kernels_of(fh.read())
        names = demangle(list(ks)) if ks else {}
        for sym, v in ks.items():
            name = unqualified(names[sym])
            if name in out:
                sys.exit("%s: two kernels named %s" % (tree, name))
            out[name] = v + (f,)
    return out


def fmt(res):
    return "/".join(str(res.get(k, "?")) for k, _ in RESOURCES)


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    tree_a, tree_b, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    files_a = files_b = files
    if "--" in files:  # the kernels moved between files: one list per tree
        files_a, files_b = files[:files.index("--")], files[files.index("--") + 1:]
    with tempfile.TemporaryDirectory() as tmpdir:
        a = compile_tree(tree_a, files_a, tmpdir, "a")
        b = compile_tree(tree_b, files_b, tmpdir, "b")
    bad = 0
    diffs = []
    print("%-44s %-10s %-22s %-22s %s" % ("kernel", "", "A vgpr/sgpr/lds/scr", "B vgpr/sgpr/lds/scr", "file A -> B"))
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("%-44s only in %s" % (name, "A" if name in a else "B"))
            bad += 1
            continue
        same = a[name][0] == b[name][0]
        where = a[name][2] if a[name][2] == b[name][2] else "%s -> %s" % (a[name][2], b[name][2])
        print("%-44s %-10s %-22s %-22s %s" % (name, "identical" if same else "DIFFERENT", fmt(a[name][1]), fmt(b[name][1]), where))
        if not same:
            bad += 1
            diffs.append("\n".join(difflib.unified_diff(a[name][0], b[name][0], "A:" + name, "B:" + name, lineterm="", n=2)))
    for d in diffs:
        print("\n" + d)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

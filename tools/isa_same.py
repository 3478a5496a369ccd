#!/usr/bin/env python3
"""developer tool: does a refactor leave the kernels' machine code as it was?  Compiles the named .hip files of two checkouts
for the device only (the Makefile's flags plus --cuda-device-only -S), cuts the assembly at the kernel labels and compares
every kernel of OLD with the kernel of NEW it is mapped to: the body and the .amdhsa_kernel descriptor, with the kernel's
own mangled name and the .LBB<n>_ / .Lfunc_end<n> numbers normalised.  It looks at nothing inside a body.
tools/isa_same.py OLD NEW bc_policy.hip bc_grad.hip ... [--map REGEX=REPL ...]   (a file missing from one tree is skipped there)
A kernel's demangled name takes the first --map rule that matches it (a refactor that renames kernels says how).  Exit
status 1 if a kernel of OLD is missing from NEW or differs."""
import os, re, subprocess, sys, tempfile

def kernels(tree, files):
    d = os.path.join(tree, "gpudrive_lab_amd", "csrc")
    flags = re.search(r"^CXXFLAGS \?= (.*)$", open(os.path.join(d, "Makefile")).read(), re.M).group(1).split()
    out = {}
    for f in files:
        if not os.path.exists(os.path.join(d, f)): continue
        with tempfile.NamedTemporaryFile(suffix=".s") as tmp:
            subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["--offload-arch=gfx950", "--cuda-device-only", "-S", f, "-o", tmp.name], cwd=d, check=True)
            asm = open(tmp.name).read()
        for sym in re.findall(r"^\s*\.amdhsa_kernel (\S+)$", asm, re.M):
            body = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(sym), asm, re.M | re.S).group(0)
            desc = re.search(r"^\s*\.amdhsa_kernel %s$.*?\.end_amdhsa_kernel" % re.escape(sym), asm, re.M | re.S).group(0)
            text = re.sub(r"\.(LBB|Lfunc_end)\d+", r".\1", (body + "\n" + desc).replace(sym[2:], "K"))
            name = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
            name = re.sub(r"gd::\(anonymous namespace\)::|^void |\(.*", "", name)
            out[f + " " + name] = [ln for ln in (re.sub(r"\s*;.*", "", ln) for ln in text.splitlines()) if ln]  # no comments
    return out


args, rules = [], []
for a in sys.argv[1:]:
    if a == "--map": continue
    (rules if "=" in a else args).append(a)
if len(args) < 3: sys.exit(__doc__)
rules = [tuple(r.split("=", 1)) for r in rules]
old, new = kernels(args[0], args[2:]), kernels(args[1], args[2:])
by_name = {k.split(" ", 1)[1]: v for k, v in new.items()}  # a kernel may have moved to another file
bad = 0
for k, body in old.items():
    name = k.split(" ", 1)[1]
    to = next((re.sub(p, r, name) for p, r in rules if re.search(p, name)), name)
    if to not in by_name:
        verdict = "MISSING"
    else:
        n = sum(a != b for a, b in zip(body, by_name[to])) + abs(len(body) - len(by_name[to]))
        verdict = "SAME" if n == 0 else "%d lines differ" % n
    bad += verdict != "SAME"
    print("%-60s %-44s %s" % (k, "" if to == name else "-> " + to, verdict))
print("%d kernels of %s, %d not the same in %s" % (len(old), args[0], bad, args[1]))
sys.exit(1 if bad else 0)

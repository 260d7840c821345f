"""Compare the ISA of the kernels of two device assemblies (hipcc --offload-arch=gfx950 --cuda-device-only -S, the Makefile's FLAGS).

usage: python tools/isa_compare.py BEFORE.s AFTER.s
       python tools/isa_compare.py --against-first NAME BEFORE.s AFTER.s

Every kernel of AFTER is compared with the kernel of the same mangled name in BEFORE, instructions and kernel descriptor, with the names
normalised: the mangled name, basic-block and temporary label numbers, comments and the section directive (a template instantiation
lives in a COMDAT section).  One line per kernel; the exit status is nonzero if a kernel differs or the two sets of kernel names differ.

--against-first NAME: every kernel of AFTER whose mangled name contains NAME is compared with the FIRST such kernel of BEFORE instead
(k_preprocess, BEFORE from a tree without the antialiased mode: the antialiased instantiation against the plain kernel; the plain
instantiation must print IDENTICAL).  The exit status follows the same rule, so it is nonzero where an instantiation differs."""
import re
import sys


def kernels(text, containing=""):
    """the kernels (the names that have a descriptor) in the order of their bodies"""
    named = set(re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M))
    return [k for k in re.findall(r"^(\w+):", text, re.M) if k in named and containing in k]


def body(text, name):
    m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end", text, re.S | re.M)
    b = re.sub(r";[^\n]*", "", m.group(1))
    b = re.sub(r"\.(LBB|Ltmp|Lfunc_end)\d+_?", r".\1N_", b)
    b = "\n".join(l for l in b.replace(name, "KERNEL").splitlines() if not l.strip().startswith((".section", ".text")))
    return b


def descriptor(text, name):
    return re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", text, re.S).group(1)


def main(argv):
    first = None
    if argv[:1] == ["--against-first"]:
        first, argv = argv[1], argv[2:]
    before, after = (open(p).read() for p in argv[:2])
    kb, ka = kernels(before, first or ""), kernels(after, first or "")
    bad = 0
    for name in ka:
        ref = kb[0] if first else name
        if ref not in kb:
            continue
        same = body(before, ref) == body(after, name) and descriptor(before, ref) == descriptor(after, name)
        bad += not same
        print(f"{name}: {'IDENTICAL' if same else 'differs'} ({len(body(after, name).splitlines())} lines)")
    if first is None:
        for name in sorted(set(kb) ^ set(ka)):
            bad += 1
            print(f"{name}: only in {'BEFORE' if name in kb else 'AFTER'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

"""Compare the ISA of k_preprocess between two device assemblies (hipcc --offload-arch=gfx950 -save-temps ... gs_preprocess.hip).

usage: python tools/isa_compare.py BEFORE.s AFTER.s

Every k_preprocess instantiation of AFTER is compared with the first k_preprocess of BEFORE, instructions and kernel descriptor, with
the names normalised: the mangled name, basic-block and temporary label numbers, comments and the section directive (a template
instantiation lives in a COMDAT section).  The default (non-antialiased) variant must print IDENTICAL."""
import re
import sys


def kernels(path):
    return re.findall(r"^(_Z\w*k_preprocess\w*):", open(path).read(), re.M)


def body(path, name):
    s = open(path).read()
    m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end", s, re.S | re.M)
    b = re.sub(r";[^\n]*", "", m.group(1))
    b = re.sub(r"\.(LBB|Ltmp|Lfunc_end)\d+_?", r".\1N_", b)
    b = "\n".join(l for l in b.replace(name, "KERNEL").splitlines() if not l.strip().startswith((".section", ".text")))
    return b


def descriptor(path, name):
    s = open(path).read()
    return re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", s, re.S).group(1)


def main(before, after):
    b = kernels(before)[0]
    for name in kernels(after):
        same = body(before, b) == body(after, name) and descriptor(before, b) == descriptor(after, name)
        print(f"{name}: {'IDENTICAL' if same else 'differs'} ({len(body(after, name).splitlines())} lines)")


if __name__ == "__main__":
    main(*sys.argv[1:3])

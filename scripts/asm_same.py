"""Which kernels of two device assemblies (`make -C cs201_sah-bvh_ray_tracer_amd/csrc asm`)
differ in their instructions: a change that adds kernels beside the frame
kernels shows with it that the existing ones still run the code they ran.

    python scripts/asm_same.py OLD/render-gfx950.s NEW/render-gfx950.s

Lists every kernel present in both files whose instruction text differs (and,
for information, the kernels only one file has). Set aside: comments,
assembler directives (the .amdhsa_ kernel descriptors and the kernarg metadata
among them), the numbering of local labels and every mangled symbol name: a
kernel is matched by its demangled name (c++filt; a template that gained an
empty trailing parameter pack mangles differently and demangles the same), and
a reference to another symbol compares as a reference. Exit status 1 if any
common kernel differs.
"""
import re
import shutil
import subprocess
import sys


def demangled(names):
    """mangled -> the name kernels are matched by."""
    filt = shutil.which("c++filt")
    if filt:
        out = subprocess.run([filt], input="\n".join(names) + "\n", capture_output=True, text=True, check=True)
        return dict(zip(names, out.stdout.split("\n")))
    # no demangler: drop an empty template parameter pack (J E) and its expansion in the parameter list (DpT<n>_)
    return {n: re.sub(r"DpT\d*_$", "", n.replace("EJEEE", "EEE")) for n in names}


def kernels(path):
    """demangled kernel name -> its normalised instruction lines."""
    text = open(path).read()
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)$", text, re.M)
    out = {}
    for name in names:
        m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S)
        if not m:
            raise SystemExit(f"{path}: no body for kernel {name}")
        lines = []
        for line in m.group(1).split("\n"):
            line = line.split(";", 1)[0].strip()
            if not line or line.startswith("."):
                # directives; a local label (.LBBn_m:) keeps its place in the text
                if not re.match(r"\.LBB\d+_\d+:", line):
                    continue
            line = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", line)
            line = re.sub(r"\b_Z\w+", "SYM", line)
            lines.append(re.sub(r"\s+", " ", line))
        out[name] = lines
    names = demangled(list(out))
    return {names[n]: lines for n, lines in out.items()}


def compare(old_path, new_path):
    """(names of common kernels that differ, names only in old, names only in new)"""
    old, new = kernels(old_path), kernels(new_path)
    common = [n for n in old if n in new]
    differ = [n for n in common if old[n] != new[n]]
    return differ, [n for n in old if n not in new], [n for n in new if n not in old], len(common)


def main(argv):
    if len(argv) != 3:
        raise SystemExit(__doc__)
    differ, gone, added, common = compare(argv[1], argv[2])
    for n in gone:
        print("only in old:", n)
    for n in added:
        print("only in new:", n)
    for n in differ:
        print("DIFFERS:", n)
    print(f"{common} kernels in both, {len(differ)} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

"""Device ISA of two source trees compared function by function (is a kernel's code unchanged?).

    python tools/isa_compare.py OTHER_TREE [file.hip ...]

Compiles each translation unit (default: every csrc/*.hip that both trees have) of this
tree and of OTHER_TREE (a checkout of the commit to compare with) to gfx950 assembly with the Makefile's
flags, and compares every function's instruction text.  Prints one line per translation unit and the names
of the functions that differ or exist on one side only (a function whose name alone changed is paired with
its twin by its text, and its callers are compared under the new name); exit status 1 if any differs."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("3ddctvideoencoding_amd", "csrc")


def functions(tree, unit, tmp):
    out = os.path.join(tmp, "isa.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                           "-fPIC", "-I" + os.path.join(tree, "include"), "--cuda-device-only", "-S", "-o", out,
                           os.path.join(tree, CSRC, unit)], stderr=subprocess.DEVNULL)
    s = open(out).read()
    fns = {}
    for m in re.finditer(r"^(_Z\S+):\s", s, re.M):
        end = s.find(".Lfunc_end", m.end())
        if end < 0:  # a data symbol after the last function
            continue
        body = s[m.end():end]
        # instructions and labels only: no comments, no directives.  A local label carries the function's place
        # in its unit's output (.LBB<place>_<block>), which changes with the order of instantiation and says
        # nothing about the function: the place is dropped, the block numbers stay.
        lines = [re.sub(r"\.L(BB|JTI)\d+_", r".L\1_", re.sub(r"\s*;.*$", "", ln)).strip() for ln in body.splitlines()]
        fns[m.group(1)] = [ln for ln in lines if ln and not ln.startswith(".") or ln.startswith(".LBB")]
    return fns


def main():
    other = os.path.abspath(sys.argv[1])
    units = sys.argv[2:] or sorted(u for u in os.listdir(os.path.join(ROOT, CSRC))
                                   if u.endswith(".hip") and os.path.exists(os.path.join(other, CSRC, u)))
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for u in units:
            a, b = functions(ROOT, u, tmp), functions(other, u, tmp)
            # a function whose name alone changed (a template parameter added with a default, a type in its
            # arguments renamed): paired with its twin by its text, and the other tree then speaks of it by its new
            # name everywhere, so that its callers do not differ by the symbol they call.  Until no pair is left: a
            # caller of a renamed function may be renamed itself.
            paired = True
            while paired:
                paired = False
                for n in sorted(set(a) - set(b)):
                    twin = [m for m in sorted(set(b) - set(a)) if [ln.replace(m, n) for ln in b[m]] == a[n]]
                    if twin:
                        print(f"    renamed, same text: {twin[0]} -> {n}")
                        b = {(n if k == twin[0] else k): [ln.replace(twin[0], n) for ln in v] for k, v in b.items()}
                        paired = True
                        break
            diff = sorted(n for n in set(a) | set(b) if a.get(n) != b.get(n))
            n_ins = sum(len(v) for v in a.values())
            print(f"{u}: {len(a)} functions, {n_ins} lines, {len(diff)} differ")
            for n in diff:
                print("   ", "only here" if n not in b else "only there" if n not in a else "differs", n)
            bad += len(diff)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

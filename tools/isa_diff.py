#!/usr/bin/env python3
"""Compare the per-kernel ISA of two `make asm` outputs (abrsimulator_amd/csrc/abr_env.s), kernel by kernel.

    python tools/isa_diff.py OLD.s NEW.s

Bodies are compared without comments, with basic-block label numbers normalised, and with the kernel's own symbol name
normalised (so that a template whose signature grew a trailing argument -- a different mangled name -- is still compared
with its old self; --strip SUFFIX removes that suffix from the new names, default: the RuleParams argument's mangling;
give it more than once to strip several, e.g. a defaulted template flag's `Lb0E` as well; --sub REGEX=REPL rewrites the
new names where removing a substring is not enough).  A template instance's
comdat `.section` directive compares equal to the plain `.text` of the function it replaced.
Prints one line per kernel that differs, every kernarg-size change, the kernels that are new, and a summary."""
import argparse
import re


def kernels(path):
    text = open(path).read()
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M):
        body = re.search(r"^" + re.escape(name) + r":(.*?)^\.Lfunc_end\d+:", text, re.S | re.M).group(1)
        lines = [re.sub(r"\s*;.*$", "", l) for l in body.splitlines()]
        body = "\n".join(l for l in lines if l.strip() and ".amdhsa_kernarg_size" not in l)   # reported on its own
        body = re.sub(r"\.LBB\d+_", ".LBB_", body)
        # a template instance is emitted into a comdat section of its own: the same code
        body = re.sub(r"^\s*\.section\s+\.text\.\S+,\"axG\",@progbits,\S+,comdat$", "\t.text", body, flags=re.M)
        desc = re.search(r"\.amdhsa_kernel\s+" + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", text, re.S).group(1)
        kernarg = int(re.search(r"\.amdhsa_kernarg_size\s+(\d+)", desc).group(1))
        out[name] = (body, kernarg)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--strip", action="append")
    ap.add_argument("--sub", action="append", default=[], metavar="REGEX=REPL",
                    help="rewrite the new names with re.sub before comparing, e.g. a new defaulted template flag in the middle")
    a = ap.parse_args()
    strips = a.strip if a.strip is not None else ["N4abrx10RuleParamsE"]
    old = kernels(a.old)
    new = {}
    for name, (body, ka) in kernels(a.new).items():
        short = name
        for suffix in strips:
            if suffix:
                short = short.replace(suffix, "")
        for rule in a.sub:
            pat, _, repl = rule.partition("=")
            short = re.sub(pat, repl, short)
        new[short] = (body.replace(name, short), ka)
    same = 0
    for name, (body, ka) in sorted(old.items()):
        if name not in new:
            print("gone   ", name)
            continue
        nbody, nka = new[name]
        if nbody == body:
            same += 1
        else:
            print("differs", name)
        if nka != ka:
            print("kernarg", name, ka, "->", nka)
    added = sorted(set(new) - set(old))
    for n in added:
        print("new    ", n)
    print(f"{same} of {len(old)} kernels identical, {len(added)} new")


if __name__ == "__main__":
    main()

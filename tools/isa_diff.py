"""Compare two gfx950 device assemblies function by function (no GPU needed).

For each `.text.<symbol>` section: the instruction text with comments dropped
and the function-numbered local labels (.LBB<n>_<m>, .Lfunc_end<n>) renumbered,
so that the order in which the compiler emitted the functions does not count;
for each kernel also its .amdhsa_* descriptor block and its amdhsa.kernels
metadata entry (registers, LDS, scratch, kernarg size). Prints the symbols
added, removed and differing; exit status 1 on any.

usage: hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S csrc/arnoldi.hip -o NEW.s
       python tools/isa_diff.py OLD.s NEW.s
"""
import re
import sys

LABEL = re.compile(r"\.L([A-Za-z]+?)\d+_(\d+)\b")
FUNC_LABEL = re.compile(r"\.Lfunc_(begin|end)\d+\b")


def parse(path):
    """{symbol: {"text": [...], "descriptor": [...], "metadata": [...]}}"""
    funcs = {}
    part = lambda sym, key: funcs.setdefault(sym, {}).setdefault(key, [])
    text_of = desc_of = meta = None
    in_meta = False
    for raw in open(path, errors="replace"):
        if in_meta:
            if raw.startswith("  - "):  # next entry of amdhsa.kernels
                meta = []
            elif not raw.startswith("    "):  # amdhsa.target, amdhsa.version, the end marker
                meta = None
            if meta is None:
                continue
            meta.append(raw.rstrip())
            m = re.match(r"    \.name:\s+(\S+)", raw)
            if m:
                part(m.group(1), "metadata")
                funcs[m.group(1)]["metadata"] = meta
            continue
        line = raw.split(";", 1)[0].strip()
        if not line:
            continue
        if line.startswith(".amdgpu_metadata"):
            in_meta = True
        elif line.startswith(".section"):
            m = re.match(r"\.section\s+\.text\.([^,\s]+)", line)
            text_of = m.group(1) if m else None
        elif line.startswith(".amdhsa_kernel"):
            desc_of = line.split()[1]
        elif line.startswith(".end_amdhsa_kernel"):
            desc_of = None
        elif desc_of:
            part(desc_of, "descriptor").append(line)
        elif text_of:
            part(text_of, "text").append(FUNC_LABEL.sub(r".Lfunc_\1", LABEL.sub(r".L\1_\2", line)))
    return funcs


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = parse(sys.argv[1]), parse(sys.argv[2])
    removed = sorted(set(old) - set(new))
    added = sorted(set(new) - set(old))
    differing = []
    for sym in sorted(set(old) & set(new)):
        parts = [k for k in ("text", "descriptor", "metadata") if old[sym].get(k) != new[sym].get(k)]
        if parts:
            differing.append(f"{sym}  ({', '.join(parts)})")
    kernels = lambda f: sum(1 for v in f.values() if "descriptor" in v)
    print(f"old: {len(old)} symbols, {kernels(old)} kernels   new: {len(new)} symbols, {kernels(new)} kernels")
    for title, syms in (("removed", removed), ("added", added), ("differing", differing)):
        print(f"{title}: {len(syms)}")
        for s in syms:
            print(f"  {s}")
    sys.exit(1 if removed or added or differing else 0)


if __name__ == "__main__":
    main()

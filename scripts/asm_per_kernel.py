"""Compare gfx950 device assembly kernel by kernel between two sets of .s files (hipcc
--cuda-device-only -S), for changes that move kernels between translation units.

usage: python scripts/asm_per_kernel.py OLD.s [OLD.s ...] -- NEW.s [NEW.s ...]

A kernel is the text from its "<name>:" label to its ".Lfunc_end" line, which holds the body and the
".amdhsa_kernel" descriptor block, plus the resource summary (.set / comment lines) after it. The
only normalisation is the function index in compiler-local labels (.LBB<n>_, .Lfunc_end<n>,
.Lfunc_begin<n>, .Ltmp<n>, and "Header=BB<n>_" in the compiler's loop comments, with the column
padding between such a label and its comment, which follows the index's digit count) and the
__hip_cuid_ lines. Prints the kernel count per file, names missing on either side or occurring twice, and the
kernels whose text differs; exit status 1 if anything differs."""
import re
import sys

LOCAL = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin|Ltmp)\d+")
HEADER = re.compile(r"Header=BB\d+_")
PAD = re.compile(r"^(\.LBBN_\d+:)\s+;")


def norm(ln):
    ln = LOCAL.sub(lambda m: "." + m.group(1) + "N", ln)
    return PAD.sub(r"\1 ;", HEADER.sub("Header=BBN_", ln))


def kernels(path):
    lines = open(path).read().split("\n")
    names = [m.group(1) for ln in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)] if m]
    out = {}
    for name in names:
        start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        assert any(".end_amdhsa_kernel" in ln for ln in lines[start:end]), name
        while re.match(r"\t\.(size|set)\s|\s*;|\s*$", lines[end + 1]):  # its resource summary
            end += 1
        text = lines[start:end + 1]
        out[name] = [norm(ln) for ln in text if "__hip_cuid_" not in ln]
    return out


def load(paths):
    allk, twice = {}, []
    for p in paths:
        ks = kernels(p)
        print(f"{len(ks):5d} kernels  {p}")
        for n, t in ks.items():
            if n in allk:
                twice.append(n)
            allk[n] = t
    return allk, twice


if __name__ == "__main__":
    sep = sys.argv.index("--")
    old, old2 = load(sys.argv[1:sep])
    new, new2 = load(sys.argv[sep + 1:])
    missing = sorted(set(old) - set(new))
    added = sorted(set(new) - set(old))
    differ = sorted(n for n in set(old) & set(new) if old[n] != new[n])
    print(f"old {len(old)} kernels, new {len(new)}; twice old {old2} new {new2}")
    print(f"missing in new: {missing}\nonly in new: {added}\ndiffering: {len(differ)}")
    for n in differ:
        nd = sum(a != b for a, b in zip(old[n], new[n])) + abs(len(old[n]) - len(new[n]))
        print(f"  {n}: {len(old[n])} / {len(new[n])} lines, {nd} differ")
    sys.exit(1 if missing or added or differ or old2 or new2 else 0)

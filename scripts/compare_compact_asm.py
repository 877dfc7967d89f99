"""Device code of the compact-scheme files, this tree against a commit, kernel by kernel (no GPU).

usage: python scripts/compare_compact_asm.py [REV] [OUTDIR]     (REV: default HEAD; OUTDIR: default
       profiles/compact_host_path)

Compiles pb_compact.hip, pb_compact_fast.hip, pb_compact_lines.hip, pb_compact_ops.hip and
pb_compact_dist.hip of REV (git archive into a temporary folder) and of the working tree with the
Makefile's flags plus --cuda-device-only -S -Rpass-analysis=kernel-resource-usage, and compares by
kernel symbol across the union of the files (a kernel that moved files still matches), as plain
text: asm_per_kernel.py's kernels() -- label to .Lfunc_end with the .amdhsa_kernel descriptor and
the resource summary, compiler-local label numbers normalised -- with comment-only and debug / line
directive lines dropped. Writes OUTDIR/asm_compare.txt (one line per kernel, `identical` or
`differs`, then the symbols only on one side) and OUTDIR/resource_usage_{parent,result}.txt (the
compiler's resource-usage remarks, one line per kernel). Exit status 1 if anything differs."""
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "scripts"))
from asm_per_kernel import kernels  # noqa: E402

FILES = ["pb_compact.hip", "pb_compact_fast.hip", "pb_compact_lines.hip", "pb_compact_ops.hip",
         "pb_compact_dist.hip"]
# poissbox_amd/csrc/Makefile: FLAGS and INC
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-Wall",
         "-Wno-unused-function"]
ROCM = os.environ.get("ROCM", "/opt/rocm")
DROP = re.compile(r"\s*(;|\.loc\s|\.file\s|\.cfi_|$)")
FIELD = re.compile(r"remark: (?:[^:]+:\d+:\d+: )?\s*([A-Za-z][A-Za-z0-9 \[\]/]*): (\S+)")


def build(tree, out):
    """-> ({kernel: text lines}, {kernel: {field: value}}) of the tree's compact files"""
    asm, usage = {}, {}
    csrc = os.path.join(tree, "poissbox_amd", "csrc")
    procs = []
    for f in FILES:
        s = os.path.join(out, f + ".s")
        cmd = [os.path.join(ROCM, "bin", "hipcc")] + FLAGS + [
            "-I" + os.path.join(tree, "include"), "-I" + os.path.join(ROCM, "include"), "-x", "hip",
            "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", f, "-o", s]
        procs.append((s, subprocess.Popen(cmd, cwd=csrc, stderr=subprocess.PIPE, text=True)))
    for s, p in procs:
        err = p.communicate()[1]
        if p.returncode:
            sys.exit(err)
        for name, text in kernels(s).items():
            assert name not in asm, name
            asm[name] = [ln for ln in text if not DROP.match(ln)]
        cur = None
        for ln in err.split("\n"):
            m = FIELD.search(ln.replace(" [-Rpass-analysis=kernel-resource-usage]", ""))
            if not m:
                continue
            if m.group(1) == "Function Name":
                cur = usage.setdefault(m.group(2), {})
            elif cur is not None:
                cur[m.group(1)] = m.group(2)
    return asm, usage


def write_usage(path, usage, names):
    with open(path, "w") as fh:
        for n in sorted(names):
            fh.write(n + "  " + "  ".join(f"{k}={v}" for k, v in usage.get(n, {}).items()) + "\n")


if __name__ == "__main__":
    rev = sys.argv[1] if len(sys.argv) > 1 else "HEAD"
    outdir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles",
                                                                "compact_host_path")
    os.makedirs(outdir, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        old_tree = os.path.join(tmp, "parent")
        os.makedirs(old_tree)
        tar = subprocess.run(["git", "-C", REPO, "archive", rev, "poissbox_amd/csrc", "include"],
                             check=True, stdout=subprocess.PIPE).stdout
        subprocess.run(["tar", "-x", "-C", old_tree], input=tar, check=True)
        for d in ("old", "new"):
            os.makedirs(os.path.join(tmp, d))
        old, old_use = build(old_tree, os.path.join(tmp, "old"))
        new, new_use = build(REPO, os.path.join(tmp, "new"))
    differs = [n for n in old if n in new and old[n] != new[n]]
    with open(os.path.join(outdir, "asm_compare.txt"), "w") as fh:
        fh.write(f"# parent {rev}: {len(old)} kernels, result: {len(new)} kernels\n")
        for n in sorted(set(old) & set(new)):
            fh.write(f"{'differs  ' if n in differs else 'identical'}  {n}\n")
        for n in sorted(set(old) - set(new)):
            fh.write(f"only in parent  {n}\n")
        for n in sorted(set(new) - set(old)):
            fh.write(f"only in result  {n}\n")
    write_usage(os.path.join(outdir, "resource_usage_parent.txt"), old_use, old)
    write_usage(os.path.join(outdir, "resource_usage_result.txt"), new_use, new)
    print(f"parent {len(old)} kernels, result {len(new)}; only in parent {len(set(old) - set(new))}, "
          f"only in result {len(set(new) - set(old))}, differing {len(differs)}")
    for n in differs:
        print("  differs:", n)
    sys.exit(1 if differs or set(old) != set(new) else 0)

"""Whether a source-only change left the device code of a kernel file as it was.

    python tools/kernel_isa_diff.py OLD.s NEW.s [--rename REGEX=REPL ...]

OLD.s / NEW.s are device assembly files as `hipcc -save-temps=obj` writes them (`*-hip-amdgcn-amd-amdhsa-gfx950.s`).  For every
kernel of either file: a digest and the line count of its body, from the kernel's label to its `.Lfunc_end` (instructions and the
kernel descriptor), and its demangled name without namespaces or parameter list.  Before hashing, everything behind `;` goes, as
do trailing blanks and empty lines, and mangled names and local labels become fixed tokens.  --rename rewrites OLD's names with
re.sub before the two sides are matched (a changed template list: --rename ', 32, 4,=,').  Reads files only; no GPU.
Exit status 1 if a kernel present in both files differs.
"""
import argparse
import hashlib
import re
import subprocess
import sys

from kernel_form_coverage import key


def kernels(path: str) -> dict:
    """{name: (digest, lines)} of every `.amdhsa_kernel` of the file"""
    text = open(path).read()
    mangled = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    names = subprocess.run(["c++filt"], input="\n".join(mangled), check=True, capture_output=True, text=True).stdout.splitlines()
    out = {}
    for sym, name in zip(mangled, names):
        body = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(sym), text, re.M | re.S).group(0).splitlines()[1:-1]
        body = [re.sub(r"_Z\w+", "SYM", re.sub(r"\.L\w+", "LABEL", ln.split(";")[0].rstrip())) for ln in body]
        body = [ln for ln in body if ln]
        out[key(name)] = (hashlib.sha256("\n".join(body).encode()).hexdigest()[:16], len(body))
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL", help="rewrite OLD's kernel names before matching")
    a = ap.parse_args(argv)
    old, new = kernels(a.old), kernels(a.new)
    for rule in a.rename:
        pat, repl = rule.split("=", 1)
        old = {re.sub(pat, repl, k): v for k, v in old.items()}
    differ = 0
    for k in sorted(set(old) | set(new)):
        o, n = old.get(k), new.get(k)
        verdict = "only old" if n is None else "only new" if o is None else "same" if o == n else "DIFFERENT"
        differ += verdict == "DIFFERENT"
        print("  ".join(f"{v[0]} {v[1]:6d}" if v else " " * 23 for v in (o, n)) + f"  {verdict:9s}  {k}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())

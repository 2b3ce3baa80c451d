"""Which device kernel instantiations of libmmfusion.so a profiled run launched, and which it never did.

    python tools/kernel_form_coverage.py LIB STATS.csv [STATS.csv ...] [--only REGEX]

LIB is the built libmmfusion.so; each STATS.csv is the kernel-stats file of a `rocprofv3 --kernel-trace --stats` run (its
`Name` column; several files are merged).  The instantiations are read off the `.kd` (kernel descriptor) symbols of the
embedded code objects with `strings` and `c++filt`, so this runs on a machine without a GPU; it reads files only.
--only keeps the instantiations whose name matches REGEX (the families a run targets, e.g. 'ln_|skinny_dgrad').
For a trace of tests/test_streaming_small_gpu.py (the kernels of elementwise.hip, small.hip and optim.hip it pins):
    --only '^(cast_|add3|addn_|relu_bwd|dropout_kernel|meanpool|colsum|zero_ranges|gat3_|nce_|ada_|attn_weights_mean|narrow_|stack3_|rowmask|sqnorm|adamw)'
For a trace of tests/test_attention_paths_gpu.py (the twelve instantiations of attention2.hip: forward, dQ and dK/dV, each at
head_dim 64 and 96, each with and without dropout; profiles/attention_form_coverage.txt):
    --only '^attn_(fwd|bwd)'    (attn_weights_mean_kernel of small.hip belongs to the streaming file's list above)
For a trace of tests/test_deberta_attention_paths_gpu.py (the forward's four and the backward's eight instantiations of deberta.hip, and the
delta pre-pass; profiles/deberta_attention_form_coverage.txt):
    --only 'deberta_attn'
Exit status 1 if an instantiation was never launched.
"""
import argparse
import csv
import re
import subprocess
import sys

def key(name: str) -> str:
    """kernel name with its template arguments, without return type, namespaces or parameter list:
    'void (anonymous namespace)::ln_fwd_kernel<1>((anonymous namespace)::LnArgs) [clone .kd]' -> 'ln_fwd_kernel<1>'"""
    n = name.replace("(anonymous namespace)::", "").replace(" [clone .kd]", "").strip()
    if n.startswith("void "):
        n = n[5:]
    depth = 0
    for i, ch in enumerate(n):          # cut at the parameter list: the first '(' outside template brackets
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            n = n[:i]
            break
    return re.sub(r"\s+", " ", n).strip()


def instantiations(lib_path: str) -> set:
    out = subprocess.run(["strings", "-a", lib_path], check=True, capture_output=True, text=True).stdout
    # strings can glue a length byte in front of a name: match the mangled symbol itself
    mangled = sorted(set(re.findall(r"_Z\w+\.kd", out)))
    demangled = subprocess.run(["c++filt"], input="\n".join(mangled), check=True, capture_output=True, text=True).stdout
    return {key(line) for line in demangled.splitlines() if line.strip()}


def launched(stats_paths) -> set:
    names = set()
    for path in stats_paths:
        with open(path, newline="") as f:
            rows = [line for line in f if not line.startswith("#")]
        for row in csv.DictReader(rows):
            if row.get("Name"):
                names.add(key(row["Name"]))
    return names


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("lib")
    ap.add_argument("stats", nargs="+")
    ap.add_argument("--only", default=None, help="regex: report only the instantiations it matches")
    a = ap.parse_args(argv)
    forms = instantiations(a.lib)
    if a.only:
        forms = {k for k in forms if re.search(a.only, k)}
    ran = launched(a.stats)
    hit = sorted(forms & ran)
    missed = sorted(forms - ran)
    print(f"{len(forms)} instantiations{' matching ' + repr(a.only) if a.only else ''}; {len(hit)} launched, "
          f"{len(missed)} never launched")
    for k in hit:
        print(f"  launched    {k}")
    for k in missed:
        print(f"  NEVER       {k}")
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())

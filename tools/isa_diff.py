"""Do two builds compile to the same device code, kernel by kernel?

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -munsafe-fp-atomics -S --cuda-device-only -o X.s X.hip
    python tools/isa_diff.py --a old/kernels_fx.s --b new/kernels_fx.s new/kernels_fxl.s ...

Each side is one or more hipcc listings; a kernel may sit in another file on the other side.  Per
kernel symbol the instruction lines (comments, directives and the __hip_cuid_* symbol dropped; block
and jump-table labels rewritten so that the function's index within its file does not show) and the
metadata (registers, spills, scratch, LDS, occupancy, kernarg layout) are compared.  Exit status 0
only if both sides hold the same kernels, no instruction line differs and all metadata is equal.
"""
import argparse
import difflib
import re
import sys

LABEL = re.compile(r"\.L(BB|JTI)\d+_(\d+)")


def kernels(path):
    """{symbol: (instruction lines, metadata lines)} of one listing"""
    lines = open(path).read().split("\n")
    names, meta, entry = [], {}, None
    for i in range(lines.index("amdhsa.kernels:") + 1, len(lines)):  # the YAML note: one entry per kernel
        l = lines[i]
        if l.startswith("  - "):
            entry = [l[4:]]
        elif l.startswith("    ") and entry is not None:
            entry.append(l[4:])
            m = re.match(r"\s+\.name:\s+(\S+)", l)
            if m:
                names.append(m.group(1))
                meta[m.group(1)] = entry
        elif not l.startswith(" "):
            break
    out = {}
    start = {l.split(":")[0]: i for i, l in enumerate(lines) if l[:1].isalpha() or l[:1] == "_"}
    for sym in names:
        at = start[sym]
        end = next(i for i in range(at, len(lines)) if lines[i].startswith(".Lfunc_end"))
        body = []
        for l in lines[at + 1:end]:
            t = l.split(";")[0].strip()
            if not t or (t.startswith(".") and not t.endswith(":")) or "__hip_cuid_" in t:
                continue
            body.append(LABEL.sub(r".L\1_\2", t))
        occ = next(l.strip("; ") for l in lines[end:end + 80] if l.startswith("; Occupancy:"))
        md = [l for l in meta[sym] if not re.match(r"\s*\.(name|symbol):", l)] + [occ]
        out[sym] = (body, md)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", nargs="+", required=True)
    ap.add_argument("--b", nargs="+", required=True)
    ap.add_argument("--show", type=int, default=0, help="print this many differing lines per kernel")
    a = ap.parse_args()
    side = []
    for files in (a.a, a.b):
        ks = {}
        for f in files:
            for sym, v in kernels(f).items():
                if sym in ks:
                    sys.exit(f"{sym} defined twice on one side")
                ks[sym] = v
        side.append(ks)
    A, B = side
    only = sorted(set(A) ^ set(B))
    for sym in only:
        print(("only in a: " if sym in A else "only in b: ") + sym)
    n_lines = n_diff = n_meta = 0
    for sym in sorted(set(A) & set(B)):
        (ia, ma), (ib, mb) = A[sym], B[sym]
        n_lines += len(ia)
        if ia != ib:
            d = [l for l in difflib.unified_diff(ia, ib, lineterm="", n=0) if l[0] in "+-" and l[:3] not in ("+++", "---")]
            n_diff += len(d)
            print(f"{sym}: {len(d)} differing instruction lines")
            for l in d[:a.show]:
                print("    " + l)
        if ma != mb:
            n_meta += 1
            print(f"{sym}: metadata differs")
            for l in difflib.unified_diff(ma, mb, lineterm="", n=0):
                if l[0] in "+-" and l[:3] not in ("+++", "---"):
                    print("    " + l)
    print(f"kernels: {len(A)} in a, {len(B)} in b, {len(only)} on one side only; {n_lines} instruction lines in a, "
          f"{n_diff} differing; {n_meta} kernels with differing metadata")
    sys.exit(0 if not only and not n_diff and not n_meta else 1)


if __name__ == "__main__":
    main()

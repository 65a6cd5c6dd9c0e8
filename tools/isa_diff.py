#!/usr/bin/env python3
"""Per-kernel comparison of two device assembly listings of rs_kernels.hip:

    hipcc $(HIPFLAGS) --cuda-device-only -S helyim_amd/csrc/rs_kernels.hip -o X.s
    tools/isa_diff.py parent.s head.s > profiles/verify/refactor_isa.md

Each listing is cut into per-symbol bodies (label to .Lfunc_end), comments and
blank lines are stripped, local labels lose the function's position in the
file (.LBB<n>_), and the bodies are compared as text. The resource
figures come from the .amdhsa_ directives and the metadata of each kernel."""
import re
import subprocess
import sys


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def parse(path):
    bodies, res, cur = {}, {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            bodies[cur] = []
            continue
        if cur and line.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur:
            # local labels carry the function's position in the file
            code = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0].strip())
            if code:
                bodies[cur].append(code)
    text = open(path).read()
    for m in re.finditer(r"\.amdhsa_kernel (\w+)(.*?)\.end_amdhsa_kernel", text, re.S):
        d = dict(re.findall(r"\.amdhsa_(\w+) (\d+)", m.group(2)))
        res[m.group(1)] = {"lds": d.get("group_segment_fixed_size", "0"),
                           "scratch": d.get("private_segment_fixed_size", "0")}
    meta = text[text.index("amdhsa.kernels:"):]
    for entry in re.split(r"\n  - ", meta):
        d = dict(re.findall(r"\n    \.(name|sgpr_count|vgpr_count):\s+(\w+)", "\n    " + entry))
        if "name" in d:
            res.setdefault(d["name"], {}).update(vgpr=d.get("vgpr_count", "?"), sgpr=d.get("sgpr_count", "?"))
    return bodies, res


def instr(body):
    return sum(1 for ln in body if not ln.endswith(":") and not ln.startswith("."))


def main():
    (pb, pr), (hb, hr) = parse(sys.argv[1]), parse(sys.argv[2])
    names = demangle(sorted(set(pb) | set(hb)))
    print("| symbol | | instructions | VGPRs | SGPRs | scratch B | LDS B |")
    print("|---|---|---|---|---|---|---|")
    # A kernel whose parameter type is spelled differently has another mangled
    # name: a parent-only symbol is paired with the one head-only symbol of the
    # same template-id (the demangled name up to its parameter list).
    head_only = {}
    for sym in set(hb) - set(pb):
        head_only.setdefault(names[sym].split("(")[0], []).append(sym)
    renamed = {}
    for sym in set(pb) - set(hb):
        twins = head_only.get(names[sym].split("(")[0], [])
        if len(twins) == 1:
            renamed[sym] = twins[0]
    for sym in sorted(names, key=names.get):
        if sym in renamed.values():
            continue
        other = renamed.get(sym, sym)
        a, b = pb.get(sym), hb.get(other)
        if a is None or b is None:
            verdict = "ONLY PARENT" if b is None else "ONLY HEAD"
        else:
            strip = lambda body, name: [ln.replace(name, "@") for ln in body]  # noqa: E731
            verdict = "SAME" if strip(a, sym) == strip(b, other) else "DIFF"
            if other != sym:
                verdict += " (parameter type respelled)"
        cells = [f"{instr(a) if a is not None else '-'} / {instr(b) if b is not None else '-'}"]
        for key in ("vgpr", "sgpr", "scratch", "lds"):
            cells.append(f"{pr.get(sym, {}).get(key, '-')} / {hr.get(other, {}).get(key, '-')}")
        print(f"| `{names[other]}` | {verdict} | " + " | ".join(cells) + " |")


if __name__ == "__main__":
    main()

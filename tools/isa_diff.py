#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel: the check of a change that must not change a kernel.

    hipcc <the Makefile's CXXFLAGS and INC> --cuda-device-only -S -o old.s csrc/srx_api.hip     # in the old tree
    hipcc <the Makefile's CXXFLAGS and INC> --cuda-device-only -S -o new.s csrc/srx_api.hip     # in the new tree
    python tools/isa_diff.py old.s new.s [-v]

Per kernel symbol (the text from its label to its .Lfunc_end<n> label -- the whole function: a kernel with an early exit has an s_endpgm in
front of its body -- comments and directives dropped, local labels renumbered) it says
  identical   the same instructions with the same operands;
  renamed     the same instructions in the same order, registers numbered differently;
  reordered   the same number of instructions and the same multiset of opcodes, in another order;
  CHANGED     anything else,
and it compares the resource figures of the kernel descriptor (VGPRs, SGPRs, scratch, LDS).  Exit status 1 when a kernel is CHANGED,
its figures differ, or a symbol exists on one side only.  -v lists every kernel that is not identical; where the listings carry the
code-object metadata, a listed kernel's line ends in its counts there (VGPRs, AGPRs, SGPRs, scratch and LDS bytes), old -> new.
"""
import collections
import re
import shutil
import subprocess
import sys

FIGURES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size", "group_segment_fixed_size")
_REGISTER = re.compile(r"\b([vsa])(\d+|\[\d+:\d+\])")
_FUNC_END = re.compile(r"\.Lfunc_end\d+:")


def kernels(text):
    """{symbol: ([instruction lines], {figure: value})} of a `hipcc -S --cuda-device-only` listing"""
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    figs = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)(.*?)^\s*\.end_amdhsa_kernel", text, re.M | re.S):
        figs[m.group(1)] = {k: v for k, v in re.findall(r"\.amdhsa_(\w+)\s+(\S+)", m.group(2)) if k in FIGURES}
    wanted, out, cur = set(names), {}, None
    for raw in text.splitlines():
        line = raw.split(";")[0].strip()
        if cur is None:
            if line.endswith(":") and line[:-1] in wanted:
                cur = line[:-1]
                out[cur] = []
            continue
        if _FUNC_END.match(line):
            cur = None
            continue
        if not line or line.startswith(".") or line.endswith(":"):
            continue
        out[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", line))
    return {n: (out.get(n, []), figs.get(n, {})) for n in names}


METADATA = (("VGPRs", "vgpr_count"), ("AGPRs", "agpr_count"), ("SGPRs", "sgpr_count"), ("scratch", "private_segment_fixed_size"),
            ("LDS", "group_segment_fixed_size"))


def metadata(text):
    """{symbol: {key: value}} of the listing's .amdgpu_metadata section (empty without one)"""
    at = text.find(".amdgpu_metadata")
    out = {}
    for blk in re.split(r"\n  - ", text[at:])[1:] if at >= 0 else ():
        name = re.search(r"^\s+\.name:\s+(\S+)", blk, re.M)
        if name and ".vgpr_count:" in blk:
            out[name.group(1)] = {k: int(m.group(1)) for _, k in METADATA for m in [re.search(rf"\.{k}:\s+(\d+)", blk)] if m}
    return out


def verdict(a, b):
    if a == b:
        return "identical"
    if len(a) == len(b):
        if [_REGISTER.sub(r"\1#", x) for x in a] == [_REGISTER.sub(r"\1#", x) for x in b]:
            return "renamed"
        if collections.Counter(x.split()[0] for x in a) == collections.Counter(x.split()[0] for x in b):
            return "reordered"
    return "CHANGED"


def demangle(names):
    try:
        out = subprocess.run([shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, (re.sub(r"\(.*", "", re.sub(r"^void ", "", o)) for o in out)))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main(argv):
    verbose = "-v" in argv
    paths = [a for a in argv if a != "-v"]
    if len(paths) != 2:
        print(__doc__)
        return 2
    texts = [open(p).read() for p in paths]
    old, new = (kernels(t) for t in texts)
    mold, mnew = (metadata(t) for t in texts)
    only = sorted(set(old) ^ set(new))
    both = [n for n in old if n in new]
    pretty = demangle(both + only)
    tally, lines, bad = collections.Counter(), [], bool(only)
    for n in both:
        (ia, fa), (ib, fb) = old[n], new[n]
        v = verdict(ia, ib)
        tally[v] += 1
        figs = "figures equal" if fa == fb else "FIGURES " + " ".join(f"{k} {fa.get(k)}->{fb.get(k)}" for k in FIGURES if fa.get(k) != fb.get(k))
        bad = bad or v == "CHANGED" or fa != fb
        if v != "identical" or fa != fb:
            lines.append(f"  {v:9s} {pretty[n]}: {len(ia)} -> {len(ib)} instructions, {figs}")
            if n in mold and n in mnew:
                lines[-1] += "; " + " ".join(f"{t} {mold[n].get(k)}->{mnew[n].get(k)}" + ("(+)" if mnew[n].get(k, 0) > mold[n].get(k, 0) else "")
                                             for t, k in METADATA)
    print(f"{len(old)} kernels in {paths[0]}, {len(new)} in {paths[1]}: " + ", ".join(f"{tally[k]} {k}" for k in ("identical", "renamed", "reordered", "CHANGED")))
    for n in only:
        print(f"  only in {paths[0] if n in old else paths[1]}: {pretty[n]}")
    if verbose or bad:
        print("\n".join(lines))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

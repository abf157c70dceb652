#!/usr/bin/env python3
"""Kernel by kernel comparison of two gfx950 device assembly files of ptmi.hip: did a change to the sources move any machine code?

usage: python scripts/kernel_isa_diff.py BEFORE.s AFTER.s

Both files come from the project's own flags, e.g. (add -DPTMI_DIAG_BUILD for the profiling build)
  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -std=c++17 -Iinclude -Iipu_path_trace_amd/csrc --cuda-device-only -S \
        -o AFTER.s ipu_path_trace_amd/csrc/ptmi.hip
Every kernel of one file is paired with one of the other: the instances of the trace, trace-paths and feature kernels through
OLD_NAMES below -- their hand-written names up to profiles/r26 against the template arguments of ptmi_trace_variant.h -- and every
other kernel by its symbol.  A kernel's text is its lines from its label to the end of its .amdhsa_kernel descriptor, with its
own symbol, the function number in local labels (.LBB12_3, .Lfunc_end12, .LJTI12_0), the compiler's comments (they name loop
headers by function number) and the section directives (a template instance lies in a section of its own) normalised away.  Nothing is searched for in the text: it is compared line for line.
Exit status 1 on a kernel whose text differs, a kernel without a partner, or unequal kernel counts.
"""
import difflib
import re
import subprocess
import sys

CAMERAS = ("", "_pose", "_lens")                              # ptvariant::Camera: BUILTIN, POSE, LENS
BOUNCES = ("", "_guide", "_lights", "_lights_plamps")         # ptvariant::Bounce: PLAIN, ENV_GUIDE, LIGHT_GUIDE, LIGHT_GUIDE_PLAMPS
GEOMETRIES = ("", "_poly", "_mesh", "_smooth", "_tex")        # ptvariant::Geometry: SPHERES, POLY, MESH, SMOOTH, TEX
TEX = len(GEOMETRIES) - 1


def _old_names():
    """{short name of a template instance: the name of the hand-written kernel it replaces}: 57 + 19 + 5 entries."""
    table = {}
    for g, geom in enumerate(GEOMETRIES):
        table["features_kernel_tex" if g == TEX else "features_kernel<%d>" % g] = "features_kernel" + geom
        for b, bounce in enumerate(BOUNCES):
            if b == 3 and g == 0:
                continue                                      # no polygon lamp without a polygon
            tail = bounce if (b, g) == (3, 1) else bounce + geom   # the one irregular name: _lights_plamps, not _lights_plamps_poly
            table["trace_paths_tex_kernel<%d>" % b if g == TEX else "trace_paths_kernel<%d, %d>" % (b, g)] = "trace_paths%s_kernel" % tail
            for c, cam in enumerate(CAMERAS):
                table["trace_kernel_tex<%d, %d>" % (c, b) if g == TEX else "trace_kernel<%d, %d, %d>" % (c, b, g)] = "trace_kernel" + cam + tail
    return table


OLD_NAMES = _old_names()
assert len(OLD_NAMES) == len(set(OLD_NAMES.values())) == 57 + 19 + 5


def short_name(demangled):
    """'void ptd::trace_kernel<2, 0, 1>(ptd::TraceParams)' -> 'trace_kernel<2, 0, 1>'"""
    return re.sub(r"^(?:void )?ptd::", "", demangled).split("(")[0]


def old_name(demangled):
    """The short name a kernel has in profiles/r15 - r26: the hand-written name of a template instance, else its own short name."""
    s = short_name(demangled)
    return OLD_NAMES.get(s, s)


def demangle(symbols):
    out = subprocess.run(["c++filt"], input="\n".join(symbols), capture_output=True, text=True, check=True).stdout.splitlines()
    return [o.strip() for o in out]


def kernels(path):
    """{pairing key: (symbol, [normalised lines])} of every kernel in the assembly file."""
    lines = open(path).read().splitlines()
    symbols = [m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m]
    start, wanted = {}, set(symbols)
    for i, l in enumerate(lines):
        m = re.match(r"(\S+):", l)
        if m and m.group(1) in wanted and m.group(1) not in start:
            start[m.group(1)] = i
    family = set(OLD_NAMES) | set(OLD_NAMES.values())
    out = {}
    for sym, name in zip(symbols, demangle(symbols)):
        i = start[sym]
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel" )
        assert any(re.match(r"\s*\.amdhsa_kernel\s+%s$" % re.escape(sym), l) for l in lines[i:end]), "descriptor of %s not behind its code" % sym
        text = []
        for l in lines[i:end + 1]:
            if re.match(r"\s*\.(section|text)\b", l):
                continue
            l = l.split(";")[0].rstrip().replace(sym, "KERNEL")   # the comments name loop headers by function number
            if l:
                text.append(re.sub(r"\.L(BB|func_end|func_begin|JTI|CPI|tmp)\d+", r".L\1N", l))
        key = old_name(name) if short_name(name) in family else sym
        assert key not in out, "two kernels named %s" % key
        out[key] = (sym, text)
    return out


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    before, after = kernels(sys.argv[1]), kernels(sys.argv[2])
    print("kernels: %d before, %d after" % (len(before), len(after)))
    unpaired = sorted(set(before) ^ set(after))
    for k in unpaired:
        print("UNPAIRED (%s only): %s" % ("before" if k in before else "after", k))
    differing = 0
    for k in sorted(set(before) & set(after)):
        a, b = before[k][1], after[k][1]
        if a != b:
            differing += 1
            print("DIFFERS: %s (%s)" % (k, after[k][0]))
            for d in list(difflib.unified_diff(a, b, "before", "after", lineterm="", n=1))[:40]:
                print("    " + d)
    renamed = sum(1 for k in before if k in after and before[k][0] != after[k][0])
    print("%d kernels paired (%d under a new symbol), %d differing, %d unpaired" % (len(set(before) & set(after)), renamed, differing, len(unpaired)))
    bad = differing or unpaired or len(before) != len(after)
    print("VERDICT: %s" % ("DIFFERENT" if bad else "identical instruction text and kernel descriptors"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

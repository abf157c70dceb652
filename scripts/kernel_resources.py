#!/usr/bin/env python3
"""Per-kernel register / LDS / spill table of the product library (hipcc -Rpass-analysis=kernel-resource-usage).

usage: python scripts/kernel_resources.py [filter-substring] [-DPTMI_DIAG_BUILD ...]
       python scripts/kernel_resources.py --step-budget [--small] [-D...]

--step-budget: the kernels a NIF step launches beside its NIF launches -- the trace kernel instances, share_*,
memo_lookup / memo_resolve / memo_expand, the fused step's share_class_*, the mapped step's class_map_* and share_raw_claim, the class level's class_* (NIF stream) and both accumulate kernels -- against what fits beside two NIF waves per SIMD
(DESIGN.md sections 4.1 and 4.2): at most 80 allocated VGPRs (2 x 216 of a SIMD's 512 are the NIF pair's; registers are
allocated in granules of 8), no scratch, at most 3 KiB of LDS.  Exit status 1 if one is over.  The opt-in trace instances that
sections 4.12 and 4.16 document as over -- the guided ones (frame slots reserved beside their SGPR spills) and the mesh ones
(94 - 102 VGPRs; spilled VGPRs in the light-guided mesh ones) -- are listed apart as known and do not fail the check.
An instance of the trace, trace-paths and feature kernel templates is printed, filtered and matched against KNOWN_OVER under the
name of the hand-written kernel it replaced (OLD_NAMES of scripts/kernel_isa_diff.py), so rows compare with profiles/r15 - r26.
--small compiles only the headers of the small kernels (pt_nif.h, pt_nif_group.h: seconds instead of minutes) and checks the
sharing, memo and accumulate kernels alone.
"""
import os
import re
import subprocess
import sys
import tempfile

from kernel_isa_diff import old_name   # an instance of the trace kernel templates under the hand-written name of profiles/r15 - r26

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ipu_path_trace_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

BUDGET_VGPRS, BUDGET_SCRATCH, BUDGET_LDS = 80, 0, 3072
VGPR_GRANULE = 8
SMALL_KERNELS = ("share_claim_kernel", "share_resolve_kernel", "share_expand_kernel", "memo_lookup_kernel", "memo_resolve_kernel",
                 "memo_expand_kernel", "class_claim_kernel", "class_resolve_kernel", "class_spread_kernel", "share_class_claim_kernel",
                 "share_class_resolve_kernel", "share_class_expand_kernel", "class_map_claim_kernel", "class_map_expand_kernel",
                 "share_raw_claim_kernel", "class_map_release_kernel", "accumulate_kernel", "accumulate4_kernel",
                 "accumulate_mapped_kernel")
# opt-in trace instances, with a guide or a mesh: over budget by the compiler's frame slots or by design, recorded in DESIGN.md 4.12 / 4.16
KNOWN_OVER = ("_guide", "_lights", "_plamps", "_mesh")


def resource_rows(source, extra=(), device_only=False):
    """[{name, VGPRs, AGPRs, ScratchSize [bytes/lane], LDS Size [bytes/block], ...}] of every kernel hipcc compiles from `source`."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
        cmd += ["-c", "--cuda-device-only"] if device_only else ["-shared", "-fPIC"]
        cmd += ["-o", os.path.join(tmp, "out"), source, "-Rpass-analysis=kernel-resource-usage"] + list(extra)
        run = subprocess.run(cmd, capture_output=True, text=True)
    if run.returncode != 0:
        sys.stderr.write(run.stderr[-4000:])
        raise SystemExit("hipcc failed (%d)" % run.returncode)
    rows, cur = [], None
    for line in run.stderr.splitlines():
        m = re.search(r"remark: (?:\s*)Function Name: (\S+)", line)
        if m:
            cur = {"mangled": m.group(1)}
            rows.append(cur)
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+(?:\[bytes/(?:block|lane)\])?): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    names = subprocess.run(["/usr/bin/c++filt"], input="\n".join(r["mangled"] for r in rows), capture_output=True, text=True).stdout.splitlines()
    for r, n in zip(rows, names):
        r["name"] = n.strip()
    return rows


def allocated_vgprs(r):
    """Registers of the unified file a wave of the kernel takes: arch VGPRs (to a multiple of 4 if AGPRs follow) + AGPRs, in granules."""
    v, a = r.get("VGPRs", 0), r.get("AGPRs", 0)
    total = v if a == 0 else (v + 3) // 4 * 4 + a
    return max(VGPR_GRANULE, (total + VGPR_GRANULE - 1) // VGPR_GRANULE * VGPR_GRANULE)


def short_name(r):
    return old_name(r["name"])


def shown_name(r):
    """The demangled name as the earlier tables print it: a template instance as 'ptd::<old name>(arguments)'."""
    n = r["name"]
    return "ptd::" + short_name(r) + n[n.index("("):] if "<" in n.split("(")[0] and "<" not in short_name(r) else n


def step_budget(small, extra):
    if small:
        with tempfile.NamedTemporaryFile("w", suffix=".hip", delete=False) as f:
            f.write('#include "pt_nif.h"\n#include "pt_nif_group.h"\n')
        try:
            rows = resource_rows(f.name, extra, device_only=True)
        finally:
            os.unlink(f.name)
    else:
        rows = resource_rows(os.path.join(CSRC, "ptmi.hip"), extra)
    listed, known = [], []
    for r in rows:
        n = short_name(r)
        if n in SMALL_KERNELS:
            listed.append(r)
        elif not small and n.startswith("trace_kernel"):
            (known if any(k in n for k in KNOWN_OVER) else listed).append(r)
    missing = [k for k in SMALL_KERNELS if k not in {short_name(r) for r in listed}]
    if missing or (not small and not any(short_name(r).startswith("trace_kernel") for r in listed)):
        raise SystemExit("kernels not found in the compiler's remarks: %s" % (", ".join(missing) or "trace_kernel*"))

    def line(r):
        alloc, scratch, lds = allocated_vgprs(r), r.get("ScratchSize [bytes/lane]", -1), r.get("LDS Size [bytes/block]", -1)
        over = alloc > BUDGET_VGPRS or scratch > BUDGET_SCRATCH or lds > BUDGET_LDS or scratch < 0 or lds < 0
        print("%-44s VGPRs %3d allocated %3d / %d  scratch %4d / %d  LDS %5d / %d  %s" % (
            short_name(r)[:44], r.get("VGPRs", -1), alloc, BUDGET_VGPRS, scratch, BUDGET_SCRATCH, lds, BUDGET_LDS, "OVER" if over else "ok"))
        return over

    print("kernels of a NIF step on the trace and accumulate streams against the budget beside two NIF waves per SIMD%s" % (
        " (small kernels only)" if small else ""))
    n_over = sum(line(r) for r in listed)
    if known:
        print("known (DESIGN.md sections 4.12, 4.16: guided and mesh trace instances; not part of the check):")
        for r in known:
            line(r)
    print("%d kernels checked, %d over budget" % (len(listed), n_over))
    return 1 if n_over else 0


def main():
    flags = [a for a in sys.argv[1:] if a in ("--step-budget", "--small")]
    flt = [a for a in sys.argv[1:] if not a.startswith("-")]
    extra = [a for a in sys.argv[1:] if a.startswith("-") and a not in flags]
    if "--step-budget" in flags:
        raise SystemExit(step_budget("--small" in flags, extra))
    for r in resource_rows(os.path.join(CSRC, "ptmi.hip"), extra):
        if flt and not any(f in shown_name(r) for f in flt):
            continue
        print("%-90s VGPR %3d AGPR %3d SGPR %3d spillV %d spillS %d scratch %d LDS %6d occ %s" % (
            shown_name(r)[:90], r.get("VGPRs", -1), r.get("AGPRs", -1), r.get("SGPRs", -1), r.get("VGPRs Spill", -1),
            r.get("SGPRs Spill", -1), r.get("ScratchSize [bytes/lane]", -1), r.get("LDS Size [bytes/block]", -1),
            r.get("Occupancy [waves/SIMD]", "?")))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Where the passes of a NIF step lie on the device, from a rocprofv3 --kernel-trace CSV of scripts/bench_nif_sharing.py.

usage: rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python scripts/bench_nif_sharing.py --modes step --warmup 2 --steps 6
       python scripts/step_timeline.py DIR [--last 6] [--label NAME] [--batches]

The trace is cut into steps at the film_accumulate launches (the script runs one after every pt_path_trace); the steps with a
claim pass are the sharing handle's, the last --last of them the timed ones.  Per step: its span (first kernel's begin to last
kernel's end), the time a NIF launch is running, the share of the step with none.  Per batch b (--batches): A(b)'s begin and
end relative to N(b+1)'s begin and end, and T(b+3)'s begin relative to A(b)'s end -- the edge that closes the ring of batch
sets.  Then per-launch means of T, claim, resolve, N, E, A and the table's clear (a fill kernel of
more than 0.2 ms), of a mapped step's raw-pair pass and release and, where the NIF stage has its class level, of its class claim, class resolve and spread passes; and for
how much of a step each stream has a kernel of the step running."""
import argparse
import csv
import glob
import os
import statistics


def load(path):
    files = [path] if os.path.isfile(path) else sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % path)
    rows = []
    with open(files[-1], newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r.get("Stream_Id", "?"), r.get("Queue_Id", "?")))
    rows.sort()
    return rows


def kind(name):
    if "film_accumulate" in name: return "film"
    if "class_map_claim" in name: return "claim"          # the mapped step's passes: C(b) is its claim; R(b), E(b) and the release
    if "share_raw_claim" in name: return "raw"
    if "class_map_expand" in name: return "expand"
    if "class_map_release" in name: return "release"
    if "share_class_claim" in name: return "claim"       # the fused step's passes: the class is claimed inside the claim pass
    if "share_class_resolve" in name: return "resolve"
    if "share_class_expand" in name: return "expand"
    if "share_claim" in name or "memo_lookup" in name: return "claim"
    if "share_resolve" in name or "memo_resolve" in name: return "resolve"
    if "class_claim" in name: return "cclaim"
    if "class_resolve" in name: return "cresolve"
    if "class_spread" in name: return "spread"
    if "share_expand" in name or "memo_expand" in name: return "expand"
    if "accumulate4_kernel" in name or "accumulate_kernel" in name or "accumulate_mapped_kernel" in name: return "acc"   # (mapped: the pass expands too)
    if "trace_kernel" in name: return "trace"
    if "nif_kernel" in name: return "nif"
    if "fill" in name.lower() or "memset" in name.lower(): return "fill"
    return "other"


def union_ms(spans):
    total, end = 0, None
    for a, b in sorted(spans):
        if end is None or a > end:
            total += b - a
            end = b
        elif b > end:
            total += b - end
            end = b
    return total / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("path")
    ap.add_argument("--last", type=int, default=6)
    ap.add_argument("--label", default="trace")
    ap.add_argument("--batches", action="store_true")
    a = ap.parse_args()
    rows = load(a.path)
    steps, cur = [], []
    for r in rows:
        if kind(r[2]) == "film":
            if cur:
                steps.append(cur)
            cur = []
        else:
            cur.append(r)
    shared = [s for s in steps if any(kind(r[2]) == "claim" for r in s)]
    print("%s: %d steps in the trace, %d with a claim pass; the last %d are the timed ones" % (a.label, len(steps), len(shared), a.last))
    timed = shared[-a.last:]
    KINDS = ("trace", "claim", "resolve", "raw", "cclaim", "cresolve", "nif", "spread", "expand", "acc", "release")
    per = {k: [] for k in KINDS + ("clear",)}
    kernel_ms, launches = [], []
    busy = {}
    streams = {k: set() for k in per}
    idle = []
    a_in_n, t_wait = [], []
    for si, s in enumerate(timed):
        by = {k: [r for r in s if kind(r[2]) == k] for k in KINDS}
        clears = [r for r in s if kind(r[2]) == "fill" and r[1] - r[0] > 200000]
        core = [r for r in s if kind(r[2]) in by]   # the step proper: its own passes (and the clears)
        t0 = min(r[0] for r in core + clears)
        t1 = max(r[1] for r in core + clears)
        span = (t1 - t0) / 1e6
        kernel_ms.append(sum(r[1] - r[0] for r in core + clears) / 1e6)
        launches.append(len(core) + len(clears))
        nif_ms = union_ms([(r[0], r[1]) for r in by["nif"]])
        idle.append(100.0 * (1.0 - nif_ms / span))
        for k in by:
            per[k] += [(r[1] - r[0]) / 1e6 for r in by[k]]
            streams[k] |= {"s%s/q%s" % (r[3], r[4]) for r in by[k]}
        per["clear"] += [(r[1] - r[0]) / 1e6 for r in clears]
        streams["clear"] |= {"s%s/q%s" % (r[3], r[4]) for r in clears}
        for q in {r[3] for r in core + clears}:
            busy.setdefault(q, []).append(100.0 * union_ms([(r[0], r[1]) for r in core + clears if r[3] == q]) / span)
        head = (by["nif"][0][0] - t0) / 1e6 if by["nif"] else 0.0
        print("%s step %d: %d batches, span %.2f ms, NIF running %.2f ms, no NIF launch running %.1f %% of the step, first N begins at %.2f ms; clears: %s"
              % (a.label, si, len(by["nif"]), span, nif_ms, idle[-1], head,
                 ", ".join("%.2f ms at %.2f" % ((r[1] - r[0]) / 1e6, (r[0] - t0) / 1e6) for r in clears) or "none"))
        if by["claim"]:
            print("%s step %d: the last claim pass ends at %.2f ms, the last trace kernel at %.2f ms" % (
                a.label, si, (max(r[1] for r in by["claim"]) - t0) / 1e6, (max(r[1] for r in by["trace"]) - t0) / 1e6))
        A, N, T = by["acc"], by["nif"], by["trace"]
        if len(A) != len(N) or len(T) != len(N):
            continue
        for b in range(len(A)):
            line = "  b=%2d A %.2f..%.2f (%.2f ms)" % (b, (A[b][0] - t0) / 1e6, (A[b][1] - t0) / 1e6, (A[b][1] - A[b][0]) / 1e6)
            if b + 1 < len(N):
                n = N[b + 1]
                nlen = n[1] - n[0]
                line += " | N(b+1) %.2f..%.2f: A begins %+.2f ms after its begin, ends %+.2f ms before its end (at %.0f %% of it)" % (
                    (n[0] - t0) / 1e6, (n[1] - t0) / 1e6, (A[b][0] - n[0]) / 1e6, (n[1] - A[b][1]) / 1e6, 100.0 * (A[b][1] - n[0]) / nlen)
                a_in_n.append(100.0 * (A[b][1] - n[0]) / nlen)
            if b + 3 < len(T):
                line += " | T(b+3) begins %+.3f ms after A ends" % ((T[b + 3][0] - A[b][1]) / 1e6)
                t_wait.append((T[b + 3][0] - A[b][1]) / 1e6)
            if a.batches:
                print(line)
    for k in KINDS + ("clear",):
        if per[k]:
            print("%s %-8s n %4d  mean per launch %.3f ms  per step %.2f ms  streams %s"
                  % (a.label, k, len(per[k]), statistics.mean(per[k]), sum(per[k]) / max(1, len(timed)), sorted(streams[k])))
    if kernel_ms:
        print("%s kernel time per step %.1f ms in %.0f launches (clears included)" % (a.label, statistics.mean(kernel_ms), statistics.mean(launches)))
    for q in sorted(busy):
        print("%s stream %s has a kernel of the step running for %.1f %% of a step on average" % (a.label, q, statistics.mean(busy[q])))
    if idle:
        print("%s no NIF launch running: min %.1f %%, mean %.1f %%, max %.1f %% of a step" % (a.label, min(idle), statistics.mean(idle), max(idle)))
    if a_in_n:
        print("%s A(b) ends at %.0f %% of N(b+1) on average (min %.0f %%, max %.0f %%; above 100: after it)" % (a.label, statistics.mean(a_in_n), min(a_in_n), max(a_in_n)))
    if t_wait:
        late = [t for t in t_wait if t < 0.05]
        print("%s T(b+3) begins within 0.05 ms of A(b)'s end (it was waiting for it) in %d of %d cases; median gap %.2f ms"
              % (a.label, len(late), len(t_wait), statistics.median(t_wait)))


if __name__ == "__main__":
    main()

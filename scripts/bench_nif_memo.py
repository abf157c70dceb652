"""Persistent NIF memo (pt_set_nif_memo) against step-scope sharing and against neither, in ONE process, modes alternating.

C2: 1104 x 1000, 300 spp per step, depth 8, synthetic 6 x 320 NIF with the urban_alley decode constants, tile-order worklist
(bench.py's shape at one GPU).  Every round runs one step in each mode (off, step, memo) on its own handle, so a drifting clock
touches all modes alike; after --warmup rounds, --steps timed rounds.  Per mode it prints one JSON line with M path-samples/s,
rows (NIF evaluations) and served paths per step, device ms per step, the memo's own passes and retain count, and whether the
film (pt_gather_hdr of the resident film after the last step) is bit-identical to off.  Then one JSON line per step index with
the three modes' rows, served and device ms side by side, so the warm-up of the memo is visible.  --configs c2,c3,c5 adds the
4K deep-path and wide-NIF shapes.  Not bench.py: the headline keeps measuring the reference's amount of work (both off).
"""
import argparse
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ipu_path_trace_amd import nif_assets, partition, ptmi  # noqa: E402

CONFIGS = {   # name: (width, height, spp, depth, hidden, layers) -- BASELINE.json's C2 / C3 / C5
    "c2": (1104, 1000, 300, 8, 320, 6),
    "c3": (3840, 2160, 64, 16, 320, 6),
    "c5": (1104, 1000, 64, 8, 1024, 8),
}
MODES = ("off", "step", "memo")


def run(name, warmup, steps, memo_gib):
    import torch
    W, H, spp, depth, hidden, nlayers = CONFIGS[name]
    meta = nif_assets.URBAN_ALLEY_META
    layers = nif_assets.synthetic_nif(hidden=hidden, layer_count=nlayers, embedding_dim=meta["embedding_dimension"],
                                      seed=2024 if hidden == 320 else 31)
    work = partition.tile_order_worklist(W, H)
    stream = torch.cuda.current_stream().cuda_stream
    handles = {}
    for mode in MODES:
        r = ptmi.Renderer(W, H, max_work_items=work.size, max_path_length=depth, stream=stream)
        r.init_nif_weights(layers, meta["embedding_dimension"], meta["max"], nif_assets.folded_mean())
        r.init_render_settings(seed=1, aa_noise_scale=0.3, fov_degrees=90.0, samples_per_step=spp)
        if mode == "step":
            r.set_nif_sharing("step")
        if mode == "memo":
            r.set_nif_memo(int(memo_gib * (1 << 30)))
        r.setup(work.copy())
        handles[mode] = r
    acc = {m: {"sec": 0.0, "paths": 0, "escaped": 0, "rows": 0, "served": 0, "overflowed": 0, "nif_ms": 0.0, "pass_ms": 0.0,
               "total_ms": 0.0} for m in MODES}
    per_step = []
    memo_last = {}
    for i in range(warmup + steps):
        row = {"config": name, "index": i + 1, "timed": i >= warmup}   # (not "step": that is a mode's key)
        for mode in MODES:
            r = handles[mode]
            t = time.perf_counter()
            r.path_trace()
            dt = time.perf_counter() - t
            r.film_accumulate()
            st, sh, me = r.stats(), r.nif_sharing_stats(), r.nif_memo_stats()
            row[mode] = {"rows": sh["evaluations"], "served": me["served"], "device_ms": round(st.total_ms, 2),
                         "Mpaths_per_s": round(st.paths / dt / 1e6, 1)}
            if mode == "memo":
                row[mode].update(occupied=me["occupied"], memo_ms=round(me["memo_ms"], 2), retains=me["retains"])
                memo_last = me
            if i < warmup:
                continue
            a = acc[mode]
            a["sec"] += dt
            a["paths"] += st.paths
            a["nif_ms"] += st.nif_ms
            a["total_ms"] += st.total_ms
            a["escaped"] += sh["escaped"]
            a["rows"] += sh["evaluations"]
            a["overflowed"] += sh["overflowed"]
            a["served"] += me["served"]
            a["pass_ms"] += me["memo_ms"] if mode == "memo" else sh["share_ms"]
        per_step.append(row)
    films = {}
    for mode in MODES:
        r = handles[mode]
        films[mode] = hashlib.sha256(r.gather_hdr(work.size, ptmi.HDR_FILM).tobytes()).hexdigest()
        r.close()
    for mode in MODES:
        a = acc[mode]
        out = {
            "config": name, "mode": mode, "width": W, "height": H, "spp": spp, "depth": depth, "nif": "%dx%d" % (nlayers, hidden),
            "timed_steps": steps, "Mpaths_per_s": round(a["paths"] / a["sec"] / 1e6, 1),
            "device_ms_per_step": round(a["total_ms"] / steps, 2),
            "escaped_per_step": a["escaped"] // steps, "rows_per_step": a["rows"] // steps,
            "served_per_step": a["served"] // steps, "overflowed_per_step": a["overflowed"] // steps,
            "nif_ms_per_step": round(a["nif_ms"] / steps, 2), "pass_ms_per_step": round(a["pass_ms"] / steps, 2),
            "film_sha256": films[mode][:16], "film_equal_to_off": films[mode] == films["off"],
        }
        if mode == "memo":
            out.update(memo_gib=memo_gib, slots=memo_last.get("slots"), retains=memo_last.get("retains"))
        print(json.dumps(out), flush=True)
    for row in per_step:
        print(json.dumps(row), flush=True)
    return all(films[m] == films["off"] for m in MODES)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--configs", default="c2")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--memo-gib", type=float, default=24.0, help="device memory of the memo (table + retain list)")
    args = ap.parse_args()
    ok = True
    for name in args.configs.split(","):
        ok = run(name, args.warmup, args.steps, args.memo_gib) and ok
    if not ok:
        raise SystemExit("film differs between modes")


if __name__ == "__main__":
    main()

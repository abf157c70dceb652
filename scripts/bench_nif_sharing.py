"""NIF-evaluation sharing (pt_set_nif_sharing) against the headline workload, in ONE process, modes alternating.

C2: 1104 x 1000, 300 spp per step, depth 8, synthetic 6 x 320 NIF with the urban_alley decode constants, tile-order worklist
(bench.py's shape at one GPU).  Every round runs one step in each mode on its own handle, so a drifting clock touches all
modes alike; after --warmup rounds, --steps timed rounds.  Prints one JSON line per mode: M path-samples/s, escaped /
evaluations / overflowed per step, NIF and sharing device ms per step, and whether the film (pt_gather_hdr of the resident
film after the last step) is bit-identical to off.  --configs c2,c3,c5 adds the 4K deep-path and wide-NIF shapes.
--modes picks among
  off, batch, step   pt_set_nif_sharing with that mode;
  default            a handle on which pt_set_nif_sharing is never called (bench.py's handle: the automatic default).
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
MODES = ("off", "batch", "step")
ALL_MODES = MODES + ("default",)


def run(name, warmup, steps, MODES=MODES):
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
        if mode != "default":
            r.set_nif_sharing(mode)
        r.setup(work.copy())
        handles[mode] = r
    acc = {m: {"sec": 0.0, "paths": 0, "escaped": 0, "evaluations": 0, "overflowed": 0, "nif_ms": 0.0, "share_ms": 0.0,
               "total_ms": 0.0, "table_slots": 0, "mlp_rows": 0, "class_alone": 0, "class_ms": 0.0, "class_slots": 0} for m in MODES}
    for i in range(warmup + steps):
        for mode in MODES:
            r = handles[mode]
            t = time.perf_counter()
            r.path_trace()
            dt = time.perf_counter() - t
            r.film_accumulate()
            if i < warmup:
                continue
            st, sh, a = r.stats(), r.nif_sharing_stats(), acc[mode]
            a["sec"] += dt
            a["paths"] += st.paths
            a["nif_ms"] += st.nif_ms
            a["total_ms"] += st.total_ms
            for k in ("escaped", "evaluations", "overflowed", "share_ms"):
                a[k] += sh[k]
            a["table_slots"] = sh["table_slots"]
            a["ran"] = sh["mode"]
            cl = r.nif_class_stats()   # the class level of the NIF stage: the rows the network really ran
            a["mlp_rows"] += cl["mlp_rows"]
            a["class_alone"] += cl["alone"]
            a["class_ms"] += cl["class_ms"]
            a["class_slots"] = cl["table_slots"]
    films = {}
    for mode in MODES:
        r = handles[mode]
        films[mode] = hashlib.sha256(r.gather_hdr(work.size, ptmi.HDR_FILM).tobytes()).hexdigest()
        r.close()
    for mode in MODES:
        a = acc[mode]
        print(json.dumps({
            "config": name, "mode": mode, "ran": a.get("ran"), "width": W, "height": H, "spp": spp, "depth": depth, "nif": "%dx%d" % (nlayers, hidden),
            "timed_steps": steps, "Mpaths_per_s": round(a["paths"] / a["sec"] / 1e6, 1),
            "device_ms_per_step": round(a["total_ms"] / steps, 2),
            "escaped_per_step": a["escaped"] // steps, "evaluations_per_step": a["evaluations"] // steps,
            "shared_fraction": round(1.0 - a["evaluations"] / a["escaped"], 4) if a["escaped"] else 0.0,
            "overflowed_per_step": a["overflowed"] // steps, "table_slots": a["table_slots"],
            "nif_ms_per_step": round(a["nif_ms"] / steps, 2), "share_ms_per_step": round(a["share_ms"] / steps, 2),
            "mlp_rows_per_step": a["mlp_rows"] // steps, "class_alone_per_step": a["class_alone"] // steps,
            "class_table_slots": a["class_slots"], "class_ms_per_step": round(a["class_ms"] / steps, 2),
            "film_sha256": films[mode][:16], "film_equal_to_off": films[mode] == films["off"],
        }), flush=True)
    return all(films[m] == films["off"] for m in MODES)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--configs", default="c2")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--modes", default=",".join(MODES), help="comma-separated, from %s; off is always run" % ", ".join(ALL_MODES))
    args = ap.parse_args()
    modes = tuple(dict.fromkeys(["off"] + args.modes.split(",")))
    if any(m not in ALL_MODES for m in modes):
        raise SystemExit("--modes: choose from %s" % ", ".join(ALL_MODES))
    ok = True
    for name in args.configs.split(","):
        ok = run(name, args.warmup, args.steps, modes) and ok
    if not ok:
        raise SystemExit("film differs between sharing modes")


if __name__ == "__main__":
    main()

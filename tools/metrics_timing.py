"""mean_coherence on the host against the device back-end on one MI355X: same process, legs alternating.

    python tools/metrics_timing.py [--reps 5] [--configs 1,2,3] [--time-limit 900] [--out profiles/device_coherence_timing.json]

Per shape (bench.py's configs: 1 = the 20NG shape, k = 20; 2 = 100k x 50k, k = 32; 3 = 1M x 100k, k = 64) the corpus is
generated on the device (Engine.generate_synthetic) and brought to the host (download_active_csr), the topics come from a
short fit, and `utils.mean_coherence(topics, X, n_words=20)` is timed with backend="host" and backend="device" -- the device
leg includes everything a caller pays: the pattern's upload, the CSC build, the two kernels, the read-back and the
logarithms.  One untimed round of each leg, then `reps` timed rounds, the legs alternating.  At config 3 only the device leg
is repeated; the host leg runs once, for the record.  The host-side top-word selection (np.argsort per topic), part of both
legs, is timed on its own as well.  Every device result is compared with the host's for equality.

The whole run is under one time limit (SIGALRM) and stops at the first step that fails."""
import argparse
import json
import os
import signal
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(values):
    return {"min": min(values), "median": statistics.median(values), "max": max(values), "runs": values}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--configs", default="1,2,3")
    ap.add_argument("--n-words", type=int, default=20)
    ap.add_argument("--fit-iters", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--time-limit", type=int, default=900, help="seconds for the whole run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_coherence_timing.json"))
    args = ap.parse_args()

    def out_of_time(signum, frame):
        raise TimeoutError("metrics_timing: the run exceeded its time limit of %d s" % args.time_limit)
    signal.signal(signal.SIGALRM, out_of_time)
    signal.alarm(args.time_limit)

    import bench
    from enstop_amd import utils
    from enstop_amd.engine import get_engine
    eng = get_engine()
    result = {"n_words": args.n_words, "reps": args.reps, "device": eng.device_info(), "shapes": {}}
    for cfg_id in [int(v) for v in args.configs.split(",")]:
        cfg = bench.CONFIGS[cfg_id]
        k = cfg["k"]
        kw = dict(bench.TOPICAL_20NG) if cfg_id == 1 else {}
        eng.generate_synthetic(cfg["n"], cfg["m"], cfg["nnz"], zipf_s=1.07, seed=args.seed, **kw)
        eng.init_factors_device(k, args.seed)
        eng.fit(n_iter=args.fit_iters, n_iter_per_test=args.fit_iters)
        T = eng.get_factors(want_u=False)[1].astype(np.float64)
        X = eng.download_active_csr()
        eng.release_scratch()
        legs = {"host": [], "device": []}
        values = {}
        for rep in range(-1, args.reps):                       # rep -1: untimed round of each leg
            for leg in ("host", "device"):
                if leg == "host" and cfg_id == 3 and rep != 0:     # config 3: one host run, for the record
                    continue
                wall, value = timed(lambda: utils.mean_coherence(T, X, n_words=args.n_words, backend=leg))
                assert utils.last_metric_path == leg, utils.last_metric_path
                values.setdefault(leg, value)
                assert value == values[leg], (leg, value, values[leg])
                if rep >= 0:
                    legs[leg].append(wall)
                print("config %d rep %2d %-6s %.4f s  mean_coherence %.12g" % (cfg_id, rep, leg, wall, value), flush=True)
        assert values["device"] == values["host"], values
        sel = [timed(lambda: [np.argsort(T[z])[-args.n_words:] for z in range(k)])[0] for _ in range(max(args.reps, 1))]
        shape = {"n": X.shape[0], "m": X.shape[1], "stored_entries": int(X.nnz), "k": k, "mean_coherence": float(values["host"]),
                 "host_s": summary(legs["host"]), "device_s": summary(legs["device"]), "top_word_selection_s": summary(sel)}
        shape["device_median_at_or_below_host_min"] = bool(shape["device_s"]["median"] <= shape["host_s"]["min"])
        shape["host_median_over_device_median"] = round(shape["host_s"]["median"] / shape["device_s"]["median"], 2)
        result["shapes"]["config%d" % cfg_id] = shape
        print(json.dumps({"config": cfg_id, **{key: shape[key] for key in shape if key != "mean_coherence"}}), flush=True)
        if args.out:                                           # written after every shape: a later failure keeps the earlier ones
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
    signal.alarm(0)


if __name__ == "__main__":
    main()

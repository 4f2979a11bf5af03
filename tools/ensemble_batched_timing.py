"""A/B of the batched ensemble members against the member contexts on one MI355X, same process, legs alternating.

    python tools/ensemble_batched_timing.py [--reps 5] [--out FILE.json]

Runs bench.py's own 20-Newsgroups-shape legs (`ensemble_20ng_shape`: 32 members x 50 iterations through
enstop_amd.ensemble_of_topics, fits/min; `ensemble_topics_estimator_20ng_shape`: EnsembleTopics itself, wall) `reps` times
each with ENSTOP_AMD_ENSEMBLE unset (contexts) and =batched, alternating, after one untimed round of both, and prints
min / median / max per leg and mode plus the ratio of the medians.  The bar DESIGN.md section 10 uses: the batched median
against the contexts' MAXIMUM."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-estimator", action="store_true")
    args = ap.parse_args()
    import bench
    import enstop_amd
    from enstop_amd import enstop_
    from enstop_amd.engine import get_engine
    eng = get_engine()
    legs = {"ensemble_20ng_shape": lambda: bench.ensemble_20ng_shape(eng, args.seed)}
    if not args.no_estimator:
        legs["ensemble_topics_estimator_20ng_shape"] = lambda: bench.ensemble_topics_estimator_20ng_shape(eng, args.seed)
    modes = {"contexts": None, "batched": "batched"}
    res = {leg: {mode: [] for mode in modes} for leg in legs}
    for rep in range(-1, args.reps):                     # rep -1: warm-up of both paths, not recorded
        for mode, value in modes.items():
            if value is None:
                os.environ.pop("ENSTOP_AMD_ENSEMBLE", None)
            else:
                os.environ["ENSTOP_AMD_ENSEMBLE"] = value
            for leg, fn in legs.items():
                r = fn()
                assert enstop_.last_ensemble_timing["path"] == mode, enstop_.last_ensemble_timing
                if rep >= 0:
                    res[leg][mode].append({"value": r["value"], "wall_s": r["wall_s"]})
                print("rep %d %-9s %-38s %10.1f %s  wall %.4f s" % (rep, mode, leg, r["value"], r["unit"].split(",")[0], r["wall_s"]),
                      flush=True)
    os.environ.pop("ENSTOP_AMD_ENSEMBLE", None)
    out = {}
    for leg in legs:
        out[leg] = {}
        for mode in modes:
            v = [x["value"] for x in res[leg][mode]]
            w = [x["wall_s"] for x in res[leg][mode]]
            out[leg][mode] = {"fits_per_min": {"min": min(v), "median": statistics.median(v), "max": max(v)},
                              "wall_s": {"min": min(w), "median": statistics.median(w), "max": max(w)}, "runs": res[leg][mode]}
        c, b = out[leg]["contexts"]["fits_per_min"], out[leg]["batched"]["fits_per_min"]
        out[leg]["batched_median_over_contexts_median"] = round(b["median"] / c["median"], 4)
        out[leg]["batched_median_beats_contexts_max"] = bool(b["median"] > c["max"])
    print(json.dumps(out, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

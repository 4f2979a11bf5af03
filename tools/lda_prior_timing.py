"""What learning the priors costs an LDA iteration, one MI355X, same process.

    python tools/lda_prior_timing.py [--configs 1,2,3] [--reps 5] [--window 1.0] [--per-test 10] [--alpha 0.1] [--eta 0.01] [--time-limit 1100] [--out profiles/lda_prior_timing_mi355x.json]

The shapes, the LDA state and the fixed-prior leg are tools/lda_timing.py's (bench.py's configs: 1 = the 20NG shape, k = 20;
2 = 100k x 50k, k = 32; 3 = 1M x 100k, k = 64; a few fused EM iterations and a few LDA iterations give the state, kept in the
engine's snapshot slot and restored before every leg).  Three legs run the same number of iterations from that state, a test of
the bound every `--per-test` iterations, a tolerance of 0 and no `change == 0` arm:

  lda       `Engine.lda_fit(alpha, eta, doc_iter=1, ...)`: two fixed scalars, the leg of tools/lda_timing.py
  every1    `Engine.lda_prior_fit(full(k, alpha), eta, learn=3, prior_start=1, prior_every=1, ...)`: behind every iteration
            k_lda_logmean and k_lda_logmean_sums on gamma and on lambda, 2 kp doubles to the host, which waits for them, and
            the two Newton iterations; k_lda_rows_v and k_lda_bound_v where the scalar form has k_lda_rows and k_lda_bound
  every10   the same with prior_every=10 (prior_start=10: an update behind every tenth iteration)

A leg is ONE call, timed with a host clock around it; the iteration count of a shape is chosen so that the fixed-prior leg lasts
about `--window` seconds.  After one untimed round the legs ALTERNATE `--reps` times; medians are reported per iteration with
every run beside them.  A separate round runs the legs for `--probe-iters` iterations with the engine's event timing on and
records the per-kernel split: k_lda_logmean's time per launch for both tables, its slab counts and the bytes it reads on paper.

The output file is written ONCE, after every requested shape has completed.  The whole run is under one time limit (SIGALRM)
and stops at the first step that fails."""
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

LOGMEAN_SLABS = 4096             # csrc/plsa_lda_prior_plan.hpp: LDA_LOGMEAN_SLABS


def summary(values):
    return {"min": min(values), "median": statistics.median(values), "max": max(values), "runs": values}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1,2,3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0, help="seconds the fixed-prior leg's timed call should last")
    ap.add_argument("--per-test", type=int, default=10, help="iterations between two tests of the bound")
    ap.add_argument("--probe-iters", type=int, default=20, help="iterations of the sizing probe and of the per-kernel round")
    ap.add_argument("--warm-iters", type=int, default=5)
    ap.add_argument("--alpha", type=float, default=0.1, help="doc_topic_prior (every component of the start)")
    ap.add_argument("--eta", type=float, default=0.01, help="topic_word_prior")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--time-limit", type=int, default=1100, help="seconds for the whole run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lda_prior_timing_mi355x.json"))
    args = ap.parse_args()

    def out_of_time(signum, frame):
        raise TimeoutError("lda_prior_timing: the run exceeded its time limit of %d s" % args.time_limit)
    signal.signal(signal.SIGALRM, out_of_time)
    signal.alarm(args.time_limit)

    import bench
    from enstop_amd.engine import PLSA_FUSED, PLSA_STOP_NO_ZERO_ARM, get_engine
    eng = get_engine()
    configs = [int(v) for v in args.configs.split(",")]
    result = {"reps": args.reps, "window_s": args.window, "iters_per_test": args.per_test, "alpha": args.alpha, "eta": args.eta,
              "doc_iter": 1, "device": eng.device_info(), "configs": configs, "shapes": {}}
    flags = PLSA_FUSED | PLSA_STOP_NO_ZERO_ARM

    def legs_of(n_iter, k):
        kw = dict(n_iter=n_iter, n_iter_per_test=args.per_test, tolerance=0.0, flags=flags)
        start = np.full(k, args.alpha)
        return {"lda": lambda: eng.lda_fit(args.alpha, args.eta, doc_iter=1, **kw)[0],
                "every1": lambda: eng.lda_prior_fit(start, args.eta, learn=3, prior_start=1, prior_every=1, doc_iter=1, **kw)[0],
                "every10": lambda: eng.lda_prior_fit(start, args.eta, learn=3, prior_start=10, prior_every=10, doc_iter=1, **kw)[0]}
    for cfg_id in configs:
        cfg = bench.CONFIGS[cfg_id]
        k = cfg["k"]
        kp = (k + 3) // 4 * 4
        topical = dict(bench.TOPICAL_20NG) if cfg_id == 1 else {}
        nnz = eng.generate_synthetic(cfg["n"], cfg["m"], cfg["nnz"], zipf_s=1.07, seed=args.seed, **topical)
        eng.init_factors_device(k, args.seed)
        eng.fit(n_iter=args.warm_iters, n_iter_per_test=args.warm_iters, tolerance=0.0, flags=PLSA_FUSED)
        eng.lda_fit(args.alpha, args.eta, n_iter=args.warm_iters, n_iter_per_test=args.warm_iters, tolerance=0.0, flags=PLSA_FUSED)
        eng.snapshot_factors()
        probe = legs_of(args.probe_iters, k)
        for leg in probe.values():                                  # first launches: code objects, structures, scratch
            eng.restore_factors()
            leg()
        eng.restore_factors()
        per_iteration = timed(probe["lda"])[0] / args.probe_iters
        n_iter = max(args.probe_iters, -(-int(args.window / per_iteration + 1) // args.per_test) * args.per_test)
        legs = legs_of(n_iter, k)
        walls = {name: [] for name in legs}
        for rep in range(-1, args.reps):                            # rep -1: the untimed round
            for name, leg in legs.items():
                eng.restore_factors()
                wall, iters = timed(leg)
                if iters != n_iter:
                    raise RuntimeError("%s leg stopped after %d of %d iterations" % (name, iters, n_iter))
                if rep >= 0:
                    walls[name].append(wall / n_iter)
                print("config %d rep %2d: %-8s %.4f ms / iteration (%d iterations, %.2f s)"
                      % (cfg_id, rep, name, 1e3 * wall / n_iter, n_iter, wall), flush=True)
        kernels = {}
        eng.timing(True)
        for name, leg in probe.items():                             # the per-kernel split, in a round of its own
            eng.restore_factors()
            eng.timing_reset()
            leg()
            kernels[name] = {kn: {"launches": cnt, "ms_per_launch": ms / cnt, "ms_per_iteration": ms / args.probe_iters}
                             for kn, (cnt, ms) in eng.timing_report().items()}
        eng.timing(False)
        # k_lda_logmean alone, per table: the diagnostic entry point forms the sums of one table when the other pointer is NULL
        eng.restore_factors()
        eng.timing(True)
        logmean, sums = {}, np.zeros(k)
        for table, rows in (("gamma", cfg["n"]), ("lambda", cfg["m"])):
            eng.timing_reset()
            for _ in range(5):
                eng._ok(eng._L.plsa_lda_prior_stats(eng._h, sums.ctypes.data if table == "gamma" else None,
                                                    sums.ctypes.data if table == "lambda" else None))
            cnt, ms = eng.timing_report()["k_lda_logmean"]
            logmean[table] = {"rows": rows, "slabs": min(LOGMEAN_SLABS, max(rows, 1)), "launches": cnt, "ms_per_launch": ms / cnt,
                              "bytes_read": 4 * kp * rows, "GBps": round(4 * kp * rows / (ms / cnt * 1e-3) / 1e9, 1)}
        eng.timing(False)
        med = {name: statistics.median(walls[name]) for name in walls}
        shape = {"n": cfg["n"], "m": cfg["m"], "stored_entries": int(nnz), "k": k, "iterations_per_call": n_iter,
                 "s_per_iteration": {name: summary(walls[name]) for name in walls},
                 "every1_over_lda": round(med["every1"] / med["lda"], 4), "every10_over_lda": round(med["every10"] / med["lda"], 4),
                 "k_lda_logmean": logmean, "kernels": kernels}
        result["shapes"]["config%d" % cfg_id] = shape
        print(json.dumps({"config": cfg_id, **{key: v for key, v in shape.items() if key != "kernels"}}), flush=True)
        print(json.dumps({"config": cfg_id, "kernels": kernels}), flush=True)
    signal.alarm(0)
    eng.release_scratch()
    if args.out:                                                    # only a completed run leaves a file
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out + ".tmp", "w") as f:
            json.dump(result, f, indent=1)
        os.replace(args.out + ".tmp", args.out)


if __name__ == "__main__":
    main()

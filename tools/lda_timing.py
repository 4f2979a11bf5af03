"""A variational Bayes LDA iteration against a plain pLSA iteration of the same build, one MI355X, same process.

    python tools/lda_timing.py [--configs 1,2,3] [--reps 5] [--window 1.0] [--per-test 10] [--alpha 0.1] [--eta 0.01] [--time-limit 1100] [--out profiles/lda_timing_mi355x.json]

Per shape (bench.py's configs: 1 = the 20NG shape, k = 20; 2 = 100k x 50k, k = 32; 3 = 1M x 100k, k = 64) the corpus is
generated on the device, a few fused EM iterations give factors that are not flat, and a few LDA iterations from those
factors (a legal state: positive where the factors are) give an LDA state, which is kept in the engine's snapshot slot.  Two
legs then run the same number of iterations from that state (restored before every leg; the plain leg's first iteration
normalises it), a test of the objective every `--per-test` iterations (10, the estimators' default), a tolerance of 0 and no
`change == 0` arm, so that no test ends a leg.  A leg is ONE call, timed with a host clock around it; the call ends in a
stream synchronise.  The iteration count of a shape is chosen so that the plain leg lasts about `--window` seconds, from the
per-iteration time of an untimed probe of `--probe-iters` iterations.

  plain   `Engine.fit(n_iter=iters, n_iter_per_test=per_test, tolerance=0)`: plsa_fit's own loop (its streams, its look-ahead,
          the likelihood riding on a pass)
  lda     `Engine.lda_fit(alpha, eta, doc_iter=1, ...)` with the same loop arguments: the tables (k_lda_rowsum,
          k_lda_topic_partial, k_lda_topic_sums, k_lda_wordmax, k_lda_tables twice), the same passes on one stream,
          k_lda_rows behind the document pass, k_col_reduce + k_lda_topics instead of the fused column tail, the bound by
          k_loglik, k_lda_bound and k_lda_shift_sum

After one untimed round of both at the full length, the legs ALTERNATE `--reps` times; medians are reported per iteration with
every run beside them.  A third, separate round runs both legs for `--probe-iters` iterations with the engine's event timing on
and records the per-kernel split (tracing slows the host: it is not part of the timed rounds).  The split shows k_lda_rows and
the following iteration's k_lda_tables on gamma as two sweeps over the same table; the bytes the new sweeps move on paper are
reported beside their measured times.

The output file is written ONCE, after every requested shape has completed: until it exists from a completed run no cost
figure is claimed anywhere.  The whole run is under one time limit (SIGALRM) and stops at the first step that fails."""
import argparse
import json
import os
import signal
import statistics
import sys
import time

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
    ap.add_argument("--configs", default="1,2,3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0, help="seconds the plain leg's timed call should last")
    ap.add_argument("--per-test", type=int, default=10, help="iterations between two tests of the objective")
    ap.add_argument("--probe-iters", type=int, default=20, help="iterations of the sizing probe and of the per-kernel round")
    ap.add_argument("--warm-iters", type=int, default=5)
    ap.add_argument("--alpha", type=float, default=0.1, help="doc_topic_prior")
    ap.add_argument("--eta", type=float, default=0.01, help="topic_word_prior")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--time-limit", type=int, default=1100, help="seconds for the whole run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lda_timing_mi355x.json"))
    args = ap.parse_args()

    def out_of_time(signum, frame):
        raise TimeoutError("lda_timing: the run exceeded its time limit of %d s" % args.time_limit)
    signal.signal(signal.SIGALRM, out_of_time)
    signal.alarm(args.time_limit)

    import bench
    from enstop_amd.engine import PLSA_FUSED, PLSA_STOP_NO_ZERO_ARM, get_engine
    eng = get_engine()
    configs = [int(v) for v in args.configs.split(",")]
    result = {"reps": args.reps, "window_s": args.window, "iters_per_test": args.per_test, "alpha": args.alpha, "eta": args.eta,
              "doc_iter": 1, "device": eng.device_info(), "configs": configs, "shapes": {}}
    flags = PLSA_FUSED | PLSA_STOP_NO_ZERO_ARM

    def legs_of(n_iter):
        kw = dict(n_iter=n_iter, n_iter_per_test=args.per_test, tolerance=0.0, flags=flags)
        return {"plain": lambda: eng.fit(**kw), "lda": lambda: eng.lda_fit(args.alpha, args.eta, doc_iter=1, **kw)}
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
        probe = legs_of(args.probe_iters)
        eng.restore_factors()
        probe["plain"]()                                            # first launches: code objects, structures, balance
        eng.restore_factors()
        per_iteration = timed(probe["plain"])[0] / args.probe_iters
        n_iter = max(args.probe_iters, -(-int(args.window / per_iteration + 1) // args.per_test) * args.per_test)
        legs = legs_of(n_iter)
        walls = {name: [] for name in legs}
        for rep in range(-1, args.reps):                            # rep -1: the untimed round
            for name, leg in legs.items():
                eng.restore_factors()
                wall, (iters, _) = timed(leg)
                if iters != n_iter:
                    raise RuntimeError("%s leg stopped after %d of %d iterations" % (name, iters, n_iter))
                if rep >= 0:
                    walls[name].append(wall / n_iter)
                print("config %d rep %2d: %-6s %.4f ms / iteration (%d iterations, %.2f s)"
                      % (cfg_id, rep, name, 1e3 * wall / n_iter, n_iter, wall), flush=True)
        kernels = {}
        eng.timing(True)
        for name, leg in probe.items():                             # the per-kernel split, in a round of its own
            eng.restore_factors()
            eng.timing_reset()
            leg()
            kernels[name] = {kn: {"launches": cnt, "ms_per_iteration": ms / args.probe_iters} for kn, (cnt, ms) in eng.timing_report().items()}
        eng.timing(False)
        plain, lda = statistics.median(walls["plain"]), statistics.median(walls["lda"])
        sweeps = {}
        # bytes on paper per iteration: k_lda_rows reads and writes gamma; k_lda_topics reads Vacc and writes lambda; k_lda_tables
        # reads gamma and lambda and writes A and B
        for kernel, rows in (("k_lda_rows", cfg["n"]), ("k_lda_topics", cfg["m"]), ("k_lda_tables", cfg["n"] + cfg["m"])):
            ms = kernels["lda"].get(kernel, {}).get("ms_per_iteration", 0.0)
            sweeps[kernel] = {"bytes_per_iteration": 8 * kp * rows, "ms_per_iteration": ms,
                              "GBps": round(8 * kp * rows / (ms * 1e-3) / 1e9, 1) if ms > 0 else None}
        shape = {"n": cfg["n"], "m": cfg["m"], "stored_entries": int(nnz), "k": k, "iterations_per_call": n_iter,
                 "plain_s_per_iteration": summary(walls["plain"]), "lda_s_per_iteration": summary(walls["lda"]),
                 "lda_over_plain": round(lda / plain, 4), "sweeps": sweeps, "kernels_ms_per_iteration": kernels}
        result["shapes"]["config%d" % cfg_id] = shape
        print(json.dumps({"config": cfg_id, **{key: v for key, v in shape.items() if key != "kernels_ms_per_iteration"}}), flush=True)
        print(json.dumps({"config": cfg_id, "kernels_ms_per_iteration": kernels}), flush=True)
    signal.alarm(0)
    eng.release_scratch()
    if args.out:                                                    # only a completed run leaves a file
        with open(args.out + ".tmp", "w") as f:
            json.dump(result, f, indent=1)
        os.replace(args.out + ".tmp", args.out)


if __name__ == "__main__":
    main()

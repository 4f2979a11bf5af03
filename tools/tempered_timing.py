"""A tempered EM iteration against a plain one of the same build, one MI355X, same process.

    python tools/tempered_timing.py [--configs 1,2,3] [--reps 5] [--iters 20] [--beta 0.9] [--time-limit 1100] [--out profiles/tempered_timing_mi355x.json]

Per shape (bench.py's configs: 1 = the 20NG shape, k = 20; 2 = 100k x 50k, k = 32; 3 = 1M x 100k, k = 64) the corpus is
generated on the device and a few fused EM iterations give factors that are not flat.  Two legs then run `--iters` iterations
from those same factors (set back with a device-side snapshot / restore before every leg), one likelihood test per call, a
tolerance of 0, timed with a host clock around the call, which ends in a stream synchronise:

  plain      `Engine.fit(n_iter=iters, n_iter_per_test=iters, tolerance=0)`: plsa_fit's own loop (its streams, its
             look-ahead, the likelihood riding on a pass)
  tempered   `Engine.fit_tempered(beta, ...)` with the same arguments: k_temper twice per iteration, the same passes on one
             stream, the likelihoods by k_loglik

After one untimed round of both, the legs ALTERNATE (plain, tempered, plain, tempered, ...) `--reps` times; medians are reported
per iteration with every run beside them.  A third, separate round runs both legs once more with the engine's event timing on
and records the per-kernel split (tracing slows the host: it is not part of the timed rounds).  The bytes k_temper moves on
paper, 8 kp (n + m) per iteration, are reported beside its measured time.

The output file is written ONCE, after every requested shape has completed: until it exists from a completed run of all three
shapes no speed figure is claimed anywhere.  The whole run is under one time limit (SIGALRM) and stops at the first step that
fails."""
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warm-iters", type=int, default=5)
    ap.add_argument("--beta", type=float, default=0.9)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--time-limit", type=int, default=1100, help="seconds for the whole run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tempered_timing_mi355x.json"))
    args = ap.parse_args()

    def out_of_time(signum, frame):
        raise TimeoutError("tempered_timing: the run exceeded its time limit of %d s" % args.time_limit)
    signal.signal(signal.SIGALRM, out_of_time)
    signal.alarm(args.time_limit)

    import bench
    from enstop_amd.engine import PLSA_FUSED, get_engine
    eng = get_engine()
    configs = [int(v) for v in args.configs.split(",")]
    result = {"reps": args.reps, "iters_per_call": args.iters, "beta": args.beta, "device": eng.device_info(), "configs": configs,
              "shapes": {}}
    kw = dict(n_iter=args.iters, n_iter_per_test=args.iters, tolerance=0.0, flags=PLSA_FUSED)
    for cfg_id in configs:
        cfg = bench.CONFIGS[cfg_id]
        k = cfg["k"]
        kp = (k + 3) // 4 * 4
        topical = dict(bench.TOPICAL_20NG) if cfg_id == 1 else {}
        nnz = eng.generate_synthetic(cfg["n"], cfg["m"], cfg["nnz"], zipf_s=1.07, seed=args.seed, **topical)
        eng.init_factors_device(k, args.seed)
        eng.fit(n_iter=args.warm_iters, n_iter_per_test=args.warm_iters, tolerance=0.0, flags=PLSA_FUSED)
        eng.snapshot_factors()
        legs = {"plain": lambda: eng.fit(**kw), "tempered": lambda: eng.fit_tempered(args.beta, **kw)}
        walls = {name: [] for name in legs}
        for rep in range(-1, args.reps):                            # rep -1: the untimed round
            for name, leg in legs.items():
                eng.restore_factors()
                wall, (iters, _) = timed(leg)
                if iters != args.iters:
                    raise RuntimeError("%s leg stopped after %d of %d iterations" % (name, iters, args.iters))
                if rep >= 0:
                    walls[name].append(wall / args.iters)
                print("config %d rep %2d: %-8s %.4f ms / iteration" % (cfg_id, rep, name, 1e3 * wall / args.iters), flush=True)
        kernels = {}
        eng.timing(True)
        for name, leg in legs.items():                              # the per-kernel split, in a round of its own
            eng.restore_factors()
            eng.timing_reset()
            leg()
            kernels[name] = {kn: {"launches": cnt, "ms_per_iteration": ms / args.iters} for kn, (cnt, ms) in eng.timing_report().items()}
        eng.timing(False)
        plain, tempered = statistics.median(walls["plain"]), statistics.median(walls["tempered"])
        temper_bytes = 8 * kp * (cfg["n"] + cfg["m"])
        temper_ms = kernels["tempered"].get("k_temper", {}).get("ms_per_iteration", 0.0)
        shape = {"n": cfg["n"], "m": cfg["m"], "stored_entries": int(nnz), "k": k,
                 "plain_s_per_iteration": summary(walls["plain"]), "tempered_s_per_iteration": summary(walls["tempered"]),
                 "tempered_over_plain": round(tempered / plain, 4),
                 "k_temper_bytes_per_iteration": temper_bytes, "k_temper_ms_per_iteration": temper_ms,
                 "k_temper_GBps": round(temper_bytes / (temper_ms * 1e-3) / 1e9, 1) if temper_ms > 0 else None,
                 "kernels_ms_per_iteration": kernels}
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

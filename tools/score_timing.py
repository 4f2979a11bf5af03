"""Per-document scoring on the device against its float64 NumPy restatement on the host, one MI355X, same process.

    python tools/score_timing.py [--configs 1,2,3] [--reps 3] [--fit-iters 10] [--time-limit 1100] [--out profiles/score_timing_mi355x.json]

Per shape (bench.py's configs: 1 = the 20NG shape, k = 20; 2 = 100k x 50k, k = 32; 3 = 1M x 100k, k = 64) the corpus is
generated on the device, a few fused EM iterations give factors that are not flat, and corpus and factors are brought to the
host.  Two legs score the same matrix under the same factors:

  device   `Engine.score_rows()`: k_score_rows over the resident corpus and factors plus the three [n] float64 read-backs
  host     the definition of include/plsa_hip_score.h in NumPy: float32 products, float64 sums, nnz * k multiply-adds, in
           blocks of entries that keep the temporaries below `--host-block-mb`

After one untimed round of both, the legs ALTERNATE (device, host, device, host, ...) `--reps` times; medians are reported with
every run beside them, and the two legs' per-document values are compared (the log-likelihood to the error model's bound).
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

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(values):
    return {"min": min(values), "median": statistics.median(values), "max": max(values), "runs": values}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def host_score_rows(X, U, V, block_entries):
    """(ll, tokens, unscored, bound) per document: float32 products, float64 sums (include/plsa_hip_score.h restated)"""
    n, k = U.shape
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(X.indptr))
    cols = X.indices
    x = X.data.astype(np.float64)
    Vt = np.ascontiguousarray(V.T)                                  # word-major, like the device
    ll, tokens, unscored, bound = (np.zeros(n) for _ in range(4))
    for a in range(0, x.shape[0], block_entries):
        b = min(a + block_entries, x.shape[0])
        r = rows[a:b]
        dot = (Vt[cols[a:b]] * U[r]).astype(np.float64).sum(1)
        xs = x[a:b]
        hit, miss = (xs > 0) & (dot > 0), (xs > 0) & (dot == 0)
        lg = np.log(dot[hit])
        ll += np.bincount(r[hit], weights=xs[hit] * lg, minlength=n)
        tokens += np.bincount(r[hit], weights=xs[hit], minlength=n)
        unscored += np.bincount(r[miss], weights=xs[miss], minlength=n)
        bound += np.bincount(r[hit], weights=xs[hit] * (4.0 * (k + 1) * 2.0 ** -24 * np.maximum(1.0, np.abs(lg))
                                                        + k * 2.0 ** -149 / dot[hit]), minlength=n)
    return ll, tokens, unscored, bound


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1,2,3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--fit-iters", type=int, default=10)
    ap.add_argument("--host-block-mb", type=int, default=2048)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--time-limit", type=int, default=1100, help="seconds for the whole run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_timing_mi355x.json"))
    args = ap.parse_args()

    def out_of_time(signum, frame):
        raise TimeoutError("score_timing: the run exceeded its time limit of %d s" % args.time_limit)
    signal.signal(signal.SIGALRM, out_of_time)
    signal.alarm(args.time_limit)

    import bench
    from enstop_amd.engine import get_engine
    eng = get_engine()
    configs = [int(v) for v in args.configs.split(",")]
    result = {"reps": args.reps, "fit_iters": args.fit_iters, "device": eng.device_info(), "configs": configs, "shapes": {}}
    for cfg_id in configs:
        cfg = bench.CONFIGS[cfg_id]
        k = cfg["k"]
        kw = dict(bench.TOPICAL_20NG) if cfg_id == 1 else {}
        eng.generate_synthetic(cfg["n"], cfg["m"], cfg["nnz"], zipf_s=1.07, seed=args.seed, **kw)
        eng.init_factors_device(k, args.seed)
        eng.fit(n_iter=args.fit_iters, n_iter_per_test=args.fit_iters, tolerance=0.0)
        X = eng.download_active_csr()
        U, V = eng.get_factors()
        block = max(1, (args.host_block_mb << 20) // (16 * k))      # float32 products + their float64 copy per entry
        device, host = [], []
        got = want = None
        for rep in range(-1, args.reps):                            # rep -1: the untimed round
            wall_d, got = timed(lambda: eng.score_rows())
            wall_h, want = timed(lambda: host_score_rows(X, U, V, block))
            if rep >= 0:
                device.append(wall_d)
                host.append(wall_h)
            print("config %d rep %2d: device %.4f s, host %.2f s" % (cfg_id, rep, wall_d, wall_h), flush=True)
        err = np.abs(got[0] - want[0])
        nz = want[3] > 0
        shape = {"n": X.shape[0], "m": X.shape[1], "stored_entries": int(X.nnz), "k": k,
                 "device_score_rows_s": summary(device), "host_float64_numpy_s": summary(host),
                 "host_over_device": round(statistics.median(host) / statistics.median(device), 1),
                 "ll_worst_error_over_bound": float((err[nz] / want[3][nz]).max()) if nz.any() else 0.0,
                 "tokens_equal": bool(np.array_equal(got[1], want[1])), "unscored_equal": bool(np.array_equal(got[2], want[2])),
                 "sum_ll": float(np.sum(got[0])), "sum_tokens": float(np.sum(got[1])), "sum_unscored": float(np.sum(got[2]))}
        result["shapes"]["config%d" % cfg_id] = shape
        print(json.dumps({"config": cfg_id, **shape}), flush=True)
        del X, U, V, got, want
    signal.alarm(0)
    if args.out:                                                    # only a completed run leaves a file
        with open(args.out + ".tmp", "w") as f:
            json.dump(result, f, indent=1)
        os.replace(args.out + ".tmp", args.out)


if __name__ == "__main__":
    main()

"""Kullback-Leibler NMF on the device against scikit-learn on the host, one MI355X, same process.

    python tools/nmf_timing.py [--configs 1,2] [--iters 50] [--host-iters 3] [--reps 3] [--time-limit 900] [--out profiles/nmf_timing_mi355x.json]

Per shape (bench.py's configs: 1 = the 20NG shape, k = 20; 2 = 100k x 50k, k = 32) the corpus is generated on the device and
brought to the host; both legs start from the same `init="random"` factors (enstop_amd.nmf.nmf_random_init), so no SVD is in
any figure.  Measured:

  device, per iteration   `Engine.nmf_fit(max_iter=iters, tol=0)` / iters: W half + H half, no objective
  device, per fit         `Engine.nmf_fit(max_iter=200, tol=1e-4)` from the same start, objective every 10 iterations
  device, refit           `Engine.nmf_fit(update_h=False, max_iter=iters, tol=0)` / iters: the combined pass
  host, per iteration     `NMF(init="custom", solver="mu", beta_loss=1, max_iter=host_iters, tol=0)` / host_iters
  yardstick               the fused EM iteration of the unchanged pLSA code on the same corpus: `Engine.fit` / iters

A host fit to tolerance is NOT run (minutes per fit); `host_fit_s_extrapolated` is the host's per-iteration time times the
device's iteration count, and is labelled as such.  After `host_iters` iterations the two legs' factors are compared
(peak relative deviation).  The whole run is under one time limit (SIGALRM) and stops at the first step that fails."""
import argparse
import json
import os
import signal
import statistics
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(values):
    return {"min": min(values), "median": statistics.median(values), "max": max(values), "runs": values}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def peak_rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-300))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1,2")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--time-limit", type=int, default=900, help="seconds for the whole run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nmf_timing_mi355x.json"))
    args = ap.parse_args()

    def out_of_time(signum, frame):
        raise TimeoutError("nmf_timing: the run exceeded its time limit of %d s" % args.time_limit)
    signal.signal(signal.SIGALRM, out_of_time)
    signal.alarm(args.time_limit)

    import bench
    from sklearn.decomposition import NMF
    from enstop_amd import nmf
    from enstop_amd.engine import get_engine
    eng = get_engine()
    result = {"iters": args.iters, "host_iters": args.host_iters, "reps": args.reps, "device": eng.device_info(), "shapes": {}}
    for cfg_id in [int(v) for v in args.configs.split(",")]:
        cfg = bench.CONFIGS[cfg_id]
        k = cfg["k"]
        kw = dict(bench.TOPICAL_20NG) if cfg_id == 1 else {}
        eng.generate_synthetic(cfg["n"], cfg["m"], cfg["nnz"], zipf_s=1.07, seed=args.seed, **kw)
        X = eng.download_active_csr()
        W0, H0 = nmf.nmf_random_init(X, k, args.seed)

        # yardstick: the fused EM iteration of the pLSA code on this corpus
        em = []
        for rep in range(-1, args.reps):
            eng.init_factors_device(k, args.seed)
            wall, _ = timed(lambda: eng.fit(n_iter=args.iters, n_iter_per_test=args.iters, tolerance=0.0))
            if rep >= 0:
                em.append(wall / args.iters)

        per_iter, refit, fits, fit_iters = [], [], [], None
        for rep in range(-1, args.reps):
            eng.nmf_set_factors(W0, H0)
            wall, _ = timed(lambda: eng.nmf_fit(max_iter=args.iters, tol=0.0))
            eng.nmf_set_factors(W0, H0)
            wall_r, _ = timed(lambda: eng.nmf_fit(update_h=False, max_iter=args.iters, tol=0.0))
            eng.nmf_set_factors(W0, H0)
            wall_f, (n_iter, errors) = timed(lambda: eng.nmf_fit(max_iter=200, tol=1e-4))
            assert fit_iters in (None, n_iter)
            fit_iters = n_iter
            if rep >= 0:
                per_iter.append(wall / args.iters)
                refit.append(wall_r / args.iters)
                fits.append(wall_f)
            print("config %d rep %2d device: %.3f ms / iteration, refit %.3f ms / iteration, fit %.4f s (%d iterations)"
                  % (cfg_id, rep, 1e3 * wall / args.iters, 1e3 * wall_r / args.iters, wall_f, n_iter), flush=True)
        eng.nmf_set_factors(W0, H0)
        eng.nmf_fit(max_iter=args.host_iters, tol=0.0)
        Wd, Hd = eng.nmf_get_factors()

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            est = NMF(n_components=k, init="custom", solver="mu", beta_loss=1, max_iter=args.host_iters, tol=0)
            wall_h, Wh = timed(lambda: est.fit_transform(X, W=W0.copy(), H=H0.copy()))
        host_iter = wall_h / args.host_iters
        print("config %d host: %.3f s / iteration" % (cfg_id, host_iter), flush=True)

        shape = {"n": X.shape[0], "m": X.shape[1], "stored_entries": int(X.nnz), "k": k,
                 "device_iteration_s": summary(per_iter), "device_refit_iteration_s": summary(refit),
                 "device_fit_s": summary(fits), "device_fit_iterations": int(fit_iters),
                 "fused_em_iteration_s": summary(em), "host_iteration_s": host_iter, "host_iterations_timed": args.host_iters,
                 "host_fit_s_extrapolated": host_iter * fit_iters,
                 "peak_rel_W_after_host_iters": peak_rel(Wd, Wh), "peak_rel_H_after_host_iters": peak_rel(Hd, est.components_)}
        shape["nmf_iteration_over_em_iteration"] = round(shape["device_iteration_s"]["median"] / shape["fused_em_iteration_s"]["median"], 2)
        shape["host_iteration_over_device_iteration"] = round(host_iter / shape["device_iteration_s"]["median"], 1)
        result["shapes"]["config%d" % cfg_id] = shape
        print(json.dumps({"config": cfg_id, **shape}), flush=True)
        if args.out:                                           # written after every shape: a later failure keeps the earlier ones
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
    signal.alarm(0)


if __name__ == "__main__":
    main()

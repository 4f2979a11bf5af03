#!/usr/bin/env python3
"""ms per EM iteration in the REFERENCE arithmetic (PLSA_REFERENCE_SUMS) with P(z|w,d) whole and under budgets of 1/2, 1/4 and
1/8 of it (plsa_set_p_budget: the documents walked in blocks), at BASELINE config 1, config 2 and the first 150 000 documents
of config 3.  Every leg runs on a context of its own: an untimed fit, then ROUNDS timed fits of ITERS iterations; one JSON line
per config with every leg's times, the blocks it ran in and the bytes allocated for P(z|w,d).

  --whole-config5 [GB]   instead: ONE iteration of the whole of config 5 under a budget of GB gigabytes (default 32)
  --out FILE             also append the lines to FILE

On a library without plsa_set_p_budget (an older commit) only the unbudgeted leg runs: the figure to compare with."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                                                          # noqa: E402
from enstop_amd.engine import Engine, PLSA_REFERENCE_SUMS             # noqa: E402

ROUNDS, ITERS = 5, 10


def arg_after(flag, default=None):
    if flag in sys.argv:
        i = sys.argv.index(flag)
        if i + 1 < len(sys.argv) and not sys.argv[i + 1].startswith("--"):
            return sys.argv[i + 1]
    return default


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    out = arg_after("--out")
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def timed_fit(eng, n_iter):
    """wall time of n_iter iterations (one likelihood per ten, the reference's default; the call ends in a device synchronise)"""
    eng.synchronize()
    t0 = time.perf_counter()
    eng.fit(None, n_iter=n_iter, n_iter_per_test=10, tolerance=0.0, e_step_thresh=1e-32, flags=PLSA_REFERENCE_SUMS)
    return (time.perf_counter() - t0) / n_iter * 1e3


def whole_config5(gb):
    cfg = bench.CONFIGS[5]
    with Engine(0) as eng:
        eng.generate_synthetic(cfg["n"], cfg["m"], cfg["nnz"], seed=0)
        n, m, nnz = eng.shape
        eng.init_factors_numpy_stream(cfg["k"], np.random.RandomState(42))
        eng.set_p_budget(int(gb * 1e9))
        ms = timed_fit(eng, 1)
        emit({"config": 5, "rows": n, "nnz": nnz, "k": cfg["k"], "whole_p_bytes": eng.p_bytes(), "budget_gb": gb,
              "ms_one_iteration_with_likelihoods": round(ms, 1), "p_block_info": eng.p_block_info()})


def main():
    if "--whole-config5" in sys.argv:
        return whole_config5(float(arg_after("--whole-config5", "32")))
    for cfg_id, rows in ((1, 0), (2, 0), (3, 150_000)):
        cfg = bench.CONFIGS[cfg_id]
        times, info, shape = {}, {}, None
        legs = [("none", 0)] + ([("1/%d" % d, d) for d in (2, 4, 8)] if hasattr(Engine, "set_p_budget") else [])
        for name, div in legs:
            # a context of its own per leg: P(z|w,d) is allocated once, in the untimed fit, and nothing a leg does (a release, a
            # regrowth, placement probes) lands in another leg's timed region -- the "none" leg is what an older commit runs
            with Engine(0) as eng:
                eng.generate_synthetic(cfg["n"], cfg["m"], cfg["nnz"], seed=0)
                if rows:
                    eng.bootstrap(np.arange(rows, dtype=np.int64))
                shape = eng.shape
                eng.init_factors_numpy_stream(cfg["k"], np.random.RandomState(42))
                whole = eng.p_bytes()
                if div:
                    eng.set_p_budget(whole // div)
                timed_fit(eng, ITERS)                                 # untimed: allocations, derived structures, code objects
                times[name] = [round(timed_fit(eng, ITERS), 3) for _ in range(ROUNDS)]
                if hasattr(eng, "p_block_info"):
                    info[name] = eng.p_block_info()
                chain = eng.reference_chain_info()
        emit({"config": cfg_id, "rows": shape[0], "nnz": shape[2], "k": cfg["k"], "whole_p_bytes": whole, "iterations_per_fit": ITERS,
              "ms_per_iteration": {name: {"median": float(np.median(t)), "min": min(t), "max": max(t), "all": t}
                                   for name, t in times.items()},
              "p_block_info": info, "norm_chain_last_leg": chain})


if __name__ == "__main__":
    main()

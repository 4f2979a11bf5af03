"""What a step of online variational Bayes LDA costs, and the blend's share of it; one MI355X, one process.

    python tools/lda_online_timing.py [--configs 1,2,3] [--batches 64,8] [--reps 3] [--doc-iter 3] [--alpha 0.1] [--eta 0.01]
                                      [--time-limit 1100] [--out profiles/lda_online_timing_mi355x.json]

Per shape (bench.py's configs: 1 = the 20NG shape, k = 20; 2 = 100k x 50k, k = 32; 3 = 1M x 100k, k = 64) the corpus is
generated on the device, brought to the host once, and cut into `n_batches` blocks of whole documents by row_ranges_by_nnz, one
context per block, as lda_fit_online cuts it.  gamma comes from the device initialisation, lambda is eta plus the initialised
topics scaled to the corpus' tokens.  After one untimed epoch (structures, allocations):

  step        an epoch with a host wait after every step, a host clock around each: ms per step (median over blocks and reps)
  epoch       an epoch enqueued without any host wait, one wait at the end: ms per epoch (what lda_fit_online runs when no
              bound is asked for)
  split       one more epoch with the engines' event timing on: per step, every kernel's time, and k_lda_online_blend's share
              with its bytes on paper, 3 m kp 4 per step, beside its time.  Tracing slows the host: it is not part of the timed
              epochs.

Beside them, in the same run and on the same blocks, two things this build shares with its parent: a step of online pLSA
(OnlineState.step with inner_iter = doc_iter - 1: as many document passes), timed like `step`; and an iteration of batch LDA
over the whole corpus on one context (Engine.lda_fit, doc_iter = 1), timed as one call of `--batch-iters` iterations.

The output file is written ONCE, after everything requested has completed: until it exists from a completed run no speed
figure is claimed anywhere.  The whole run is under one time limit (SIGALRM) and stops at the first step that fails."""
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

BLEND = "k_lda_online_blend"
UPDATE = (BLEND, "k_lda_topic_sums", "k_lda_wordmax")


def summary(values):
    return {"min": min(values), "median": statistics.median(values), "max": max(values), "n": len(values)}


def time_shape(args, eng, cfg_id, n_batches):
    import bench
    from enstop_amd.engine import Engine, PLSA_FUSED
    from enstop_amd.lda_online import LdaOnlineState
    from enstop_amd.online import OnlineSchedule, OnlineState, block_tokens
    from enstop_amd.sharded import row_ranges_by_nnz
    cfg = bench.CONFIGS[cfg_id]
    k, m, n = cfg["k"], cfg["m"], cfg["n"]
    kp = (k + 3) // 4 * 4
    topical = dict(bench.TOPICAL_20NG) if cfg_id == 1 else {}
    eng.generate_synthetic(n, m, cfg["nnz"], zipf_s=1.07, seed=args.seed, **topical)
    X = eng.download_active_csr()
    eng.init_factors_device(k, args.seed)
    _, V0 = eng.get_factors(want_u=False)
    lam0 = (args.eta + V0.astype(np.float64) * (float(X.sum()) / k)).astype(np.float32)
    ranges = row_ranges_by_nnz(X.indptr, n_batches)
    engines, state, plain = [], None, None
    try:
        for i, (a, b) in enumerate(ranges):
            e = Engine(eng.device)
            engines.append(e)
            e.upload_csr(X[a:b])
            e.init_factors_device(k, args.seed + 1 + i)
        state = LdaOnlineState(eng, m, k).set_lambda(lam0)
        schedule = OnlineSchedule(n_batches, 10 ** 6, tolerance=0.0)

        def epoch(wait_each):
            walls = []
            for e, (a, b) in zip(engines, ranges):
                _, _, rho = schedule.next_step()
                t0 = time.perf_counter()
                state.step(e, args.alpha, args.eta, rho, float(n) / (b - a), args.doc_iter, flags=PLSA_FUSED)
                if wait_each:
                    e.synchronize()
                    walls.append(time.perf_counter() - t0)
            engines[-1].synchronize()
            schedule.end_epoch(float("nan"))
            return walls

        epoch(True)                                                  # untimed
        step_walls, epoch_walls = [], []
        for _ in range(args.reps):
            step_walls += epoch(True)
            t0 = time.perf_counter()
            epoch(False)
            epoch_walls.append(time.perf_counter() - t0)
        for e in engines:
            e.timing(True)
            e.timing_reset()
        epoch(True)
        kernels = {}
        for e in engines:
            for name, (cnt, ms) in e.timing_report().items():
                kernels[name] = kernels.get(name, 0.0) + ms / n_batches
            e.timing(False)
        total_ms = sum(kernels.values())
        blend_ms = kernels.get(BLEND, 0.0)
        blend_bytes = 3 * m * kp * 4
        out = {"config": cfg_id, "n": n, "m": m, "k": k, "stored_entries": int(X.nnz), "n_batches": n_batches,
               "doc_iter": args.doc_iter, "alpha": args.alpha, "eta": args.eta,
               "s_per_step": summary(step_walls), "s_per_epoch": summary(epoch_walls), "kernels_ms_per_step": kernels,
               "kernel_ms_per_step": total_ms, "blend_ms_per_step": blend_ms,
               "blend_share_of_kernel_time": round(blend_ms / total_ms, 4) if total_ms > 0 else None,
               "update_ms_per_step_without_the_table": sum(kernels.get(name, 0.0) for name in UPDATE),
               "blend_bytes_per_step": blend_bytes,
               "blend_GBps": round(blend_bytes / (blend_ms * 1e-3) / 1e9, 1) if blend_ms > 0 else None,
               "bytes_per_block_context": 3 * 4 * m * kp}
        # a step of online pLSA on the same blocks: normalised factors, as many document passes
        for i, e in enumerate(engines):
            e.init_factors_device(k, args.seed + 1 + i)
        plain = OnlineState(eng, m, k).set_topics(V0)
        scales = [1.0 / block_tokens(X[a:b]) for a, b in ranges]

        def plain_epoch():
            walls = []
            for e, scale in zip(engines, scales):
                _, _, rho = schedule.next_step()
                t0 = time.perf_counter()
                plain.step(e, rho, scale, args.doc_iter - 1, flags=PLSA_FUSED)
                e.synchronize()
                walls.append(time.perf_counter() - t0)
            schedule.end_epoch(float("nan"))
            return walls

        plain_epoch()                                                # untimed
        plain_walls = []
        for _ in range(args.reps):
            plain_walls += plain_epoch()
        out["plsa_online_s_per_step"] = summary(plain_walls)
        out["lda_over_plsa_step"] = round(out["s_per_step"]["median"] / out["plsa_online_s_per_step"]["median"], 4)
    finally:
        for s in (state, plain):
            if s is not None:
                s.close()
        for e in engines:
            e.close()
    return out


def time_batch(args, eng, cfg_id):
    """an iteration of batch LDA over the whole corpus of the shape, on the home context (the corpus is still resident)"""
    import bench
    from enstop_amd.engine import PLSA_FUSED, PLSA_STOP_NO_ZERO_ARM
    k = bench.CONFIGS[cfg_id]["k"]
    eng.init_factors_device(k, args.seed)
    kw = dict(n_iter_per_test=args.batch_iters, tolerance=0.0, flags=PLSA_FUSED | PLSA_STOP_NO_ZERO_ARM)
    eng.lda_fit(args.alpha, args.eta, n_iter=2, **kw)               # untimed: structures, allocations, a legal LDA state
    walls = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        iters, _ = eng.lda_fit(args.alpha, args.eta, n_iter=args.batch_iters, **kw)
        walls.append((time.perf_counter() - t0) / args.batch_iters)
        if iters != args.batch_iters:
            raise RuntimeError("the batch leg stopped after %d of %d iterations" % (iters, args.batch_iters))
    return {"config": cfg_id, "iterations_per_call": args.batch_iters, "doc_iter": 1, "s_per_iteration": summary(walls)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1,2,3")
    ap.add_argument("--batches", default="64,8")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--doc-iter", type=int, default=3)
    ap.add_argument("--batch-iters", type=int, default=10)
    ap.add_argument("--alpha", type=float, default=0.1, help="doc_topic_prior")
    ap.add_argument("--eta", type=float, default=0.01, help="topic_word_prior")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--time-limit", type=int, default=1100, help="seconds for the whole run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lda_online_timing_mi355x.json"))
    args = ap.parse_args()

    def out_of_time(signum, frame):
        raise TimeoutError("lda_online_timing: the run exceeded its time limit of %d s" % args.time_limit)
    signal.signal(signal.SIGALRM, out_of_time)
    signal.alarm(args.time_limit)

    from enstop_amd.engine import get_engine
    eng = get_engine()
    configs = [int(v) for v in args.configs.split(",") if v]
    batches = [int(v) for v in args.batches.split(",") if v]
    result = {"reps": args.reps, "device": eng.device_info(), "configs": configs, "batches": batches, "steps": [],
              "batch_lda": []}
    for cfg_id in configs:
        for n_batches in batches:
            shape = time_shape(args, eng, cfg_id, n_batches)
            result["steps"].append(shape)
            print(json.dumps(shape), flush=True)
        result["batch_lda"].append(time_batch(args, eng, cfg_id))
        print(json.dumps(result["batch_lda"][-1]), flush=True)
    signal.alarm(0)
    eng.release_scratch()
    if args.out:                                                    # only a completed run leaves a file
        with open(args.out + ".tmp", "w") as f:
            json.dump(result, f, indent=1)
        os.replace(args.out + ".tmp", args.out)


if __name__ == "__main__":
    main()

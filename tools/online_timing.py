"""What a step of online EM costs, and how soon it reaches the held-out perplexity of the default fit; one MI355X, one process.

    python tools/online_timing.py [--configs 2,3] [--batches 8,64] [--reps 3] [--inner-iter 3] [--topical-n 200000]
                                  [--time-limit 1100] [--out profiles/online_timing_mi355x.json]

Per shape (bench.py's configs: 2 = 100k x 50k, k = 32; 3 = 1M x 100k, k = 64) the corpus is generated on the device, brought to
the host once, and cut into `n_batches` blocks of whole documents by row_ranges_by_nnz, one context per block, as
plsa_fit_online cuts it.  Factors come from the device initialisation.  After one untimed epoch (structures, allocations):

  step        an epoch with a host wait after every step, a host clock around each: ms per step (median over blocks and reps)
  epoch       an epoch enqueued without any host wait, one wait at the end: ms per epoch (what plsa_fit_online runs when no
              likelihood is asked for)
  split       one more epoch with the engines' event timing on: per step, the passes (k_row_pass, k_col_pass, k_col_reduce)
              against the global update (k_online_blend, k_colsum_final, k_v_normalise), with the update's bytes on paper,
              5 m kp 4 per step, beside its time.  Tracing slows the host: it is not part of the timed epochs.

Then, on the topical generator (bench.py --topics 64's corpus) at `--topical-n` documents: a tenth of every document's tokens is
held out; plsa_fit on the observed part at its default stop gives a held-out perplexity and a wall time; plsa_fit_online runs
with 1, 2, ... epochs (each a fresh call, timed whole) until its held-out perplexity is at most that figure.  Both perplexities
are taken on the host in float64 from the returned factors and are not part of the timed calls.

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

UPDATE = ("k_online_blend", "k_colsum_final", "k_v_normalise")


def summary(values):
    return {"min": min(values), "median": statistics.median(values), "max": max(values), "n": len(values)}


def held_out_perplexity(held, scored, U, V):
    rows = np.repeat(np.arange(held.shape[0]), np.diff(held.indptr))
    use = scored[rows] & (held.data > 0)
    rows, cols, x = rows[use], held.indices[use], held.data[use].astype(np.float64)
    total, ll = 0.0, 0.0
    for lo in range(0, rows.shape[0], 1 << 20):                     # in pieces: [nnz, k] float64 at once would not fit
        r, c, w = rows[lo:lo + (1 << 20)], cols[lo:lo + (1 << 20)], x[lo:lo + (1 << 20)]
        dot = np.einsum("ij,ij->i", U[r].astype(np.float64), V[:, c].T.astype(np.float64))
        ok = dot > 0
        ll += float((w[ok] * np.log(dot[ok])).sum())
        total += float(w[ok].sum())
    return float(np.exp(-ll / total))


def time_shape(args, eng, cfg_id, n_batches):
    import bench
    from enstop_amd.engine import Engine, PLSA_FUSED
    from enstop_amd.online import OnlineSchedule, OnlineState, block_tokens
    from enstop_amd.sharded import row_ranges_by_nnz
    cfg = bench.CONFIGS[cfg_id]
    k, m = cfg["k"], cfg["m"]
    kp = (k + 3) // 4 * 4
    eng.generate_synthetic(cfg["n"], m, cfg["nnz"], zipf_s=1.07, seed=args.seed)
    X = eng.download_active_csr()
    eng.init_factors_device(k, args.seed)
    _, V0 = eng.get_factors(want_u=False)
    ranges = row_ranges_by_nnz(X.indptr, n_batches)
    engines, state = [], None
    try:
        scales = []
        for a, b in ranges:
            e = Engine(eng.device)
            engines.append(e)
            e.upload_csr(X[a:b])
            e.init_factors_device(k, args.seed + 1 + len(scales))
            scales.append(1.0 / block_tokens(X[a:b]))
        state = OnlineState(eng, m, k).set_topics(V0)
        schedule = OnlineSchedule(n_batches, 10 ** 6, tolerance=0.0)

        def epoch(wait_each):
            walls = []
            for e, scale in zip(engines, scales):
                _, _, rho = schedule.next_step()
                t0 = time.perf_counter()
                state.step(e, rho, scale, args.inner_iter, flags=PLSA_FUSED)
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
        passes_ms, update_ms, kernels = 0.0, 0.0, {}
        for e in engines:
            for name, (cnt, ms) in e.timing_report().items():
                kernels[name] = kernels.get(name, 0.0) + ms / n_batches
                if name in UPDATE:
                    update_ms += ms / n_batches
                else:
                    passes_ms += ms / n_batches
            e.timing(False)
        update_bytes = 5 * m * kp * 4
        return {"config": cfg_id, "n": cfg["n"], "m": m, "k": k, "stored_entries": int(X.nnz), "n_batches": n_batches,
                "inner_iter": args.inner_iter, "s_per_step": summary(step_walls), "s_per_epoch": summary(epoch_walls),
                "passes_ms_per_step": passes_ms, "update_ms_per_step": update_ms, "update_bytes_per_step": update_bytes,
                "update_GBps": round(update_bytes / (update_ms * 1e-3) / 1e9, 1) if update_ms > 0 else None,
                "kernels_ms_per_step": kernels, "bytes_per_block_context": 3 * 4 * m * kp}
    finally:
        if state is not None:
            state.close()
        for e in engines:
            e.close()


def time_to_perplexity(args, eng):
    import bench
    from enstop_amd import plsa_fit, plsa_fit_online, split_documents
    cfg = bench.CONFIGS[3]
    n = args.topical_n
    m, k = cfg["m"], cfg["k"]
    nnz = int(cfg["nnz"] * n / cfg["n"])
    eng.generate_synthetic(n, m, nnz, zipf_s=1.07, seed=args.seed, **bench.TOPICAL)
    X = eng.download_active_csr()
    observed, held = split_documents(X, 0.9, np.random.RandomState(args.seed))
    scored = (np.diff(observed.indptr) > 0) & (np.diff(held.indptr) > 0)
    plsa_fit(observed, k, None, n_iter=2, random_state=args.seed)                      # untimed: structures, allocations
    t0 = time.perf_counter()
    U, V, info = plsa_fit(observed, k, None, random_state=args.seed, return_info=True)
    batch_s = time.perf_counter() - t0
    target = held_out_perplexity(held, scored, U, V)
    out = {"n": n, "m": m, "k": k, "stored_entries": int(X.nnz), "topics": bench.TOPICAL,
           "plsa_fit": {"seconds": batch_s, "iterations": int(info["n_iter"]), "held_out_perplexity": target}, "online": []}
    print(json.dumps(out["plsa_fit"]), flush=True)
    for epochs in range(1, args.max_epochs + 1):
        t0 = time.perf_counter()
        U, V = plsa_fit_online(observed, k, n_batches=args.topical_batches, n_epochs=epochs, inner_iter=args.inner_iter,
                               tolerance=0.0, random_state=args.seed)
        seconds = time.perf_counter() - t0
        perplexity = held_out_perplexity(held, scored, U, V)
        out["online"].append({"epochs": epochs, "seconds": seconds, "held_out_perplexity": perplexity})
        print(json.dumps(out["online"][-1]), flush=True)
        if perplexity <= target:
            break
    out["reached"] = out["online"][-1]["held_out_perplexity"] <= target
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,3")
    ap.add_argument("--batches", default="8,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner-iter", type=int, default=3)
    ap.add_argument("--topical-n", type=int, default=200_000, help="documents of the time-to-perplexity corpus (0: skip it)")
    ap.add_argument("--topical-batches", type=int, default=64)
    ap.add_argument("--max-epochs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--time-limit", type=int, default=1100, help="seconds for the whole run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "online_timing_mi355x.json"))
    args = ap.parse_args()

    def out_of_time(signum, frame):
        raise TimeoutError("online_timing: the run exceeded its time limit of %d s" % args.time_limit)
    signal.signal(signal.SIGALRM, out_of_time)
    signal.alarm(args.time_limit)

    from enstop_amd.engine import get_engine
    eng = get_engine()
    configs = [int(v) for v in args.configs.split(",") if v]
    batches = [int(v) for v in args.batches.split(",") if v]
    result = {"reps": args.reps, "device": eng.device_info(), "configs": configs, "batches": batches, "steps": []}
    for cfg_id in configs:
        for n_batches in batches:
            shape = time_shape(args, eng, cfg_id, n_batches)
            result["steps"].append(shape)
            print(json.dumps(shape), flush=True)
    if args.topical_n > 0:
        result["time_to_perplexity"] = time_to_perplexity(args, eng)
    signal.alarm(0)
    eng.release_scratch()
    if args.out:                                                    # only a completed run leaves a file
        with open(args.out + ".tmp", "w") as f:
            json.dump(result, f, indent=1)
        os.replace(args.out + ".tmp", args.out)


if __name__ == "__main__":
    main()

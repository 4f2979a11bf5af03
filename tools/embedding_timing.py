"""Stage times of the native embedding behind topic_combination="hellinger_umap"  at t = 160 / 640 /
2560 stacked topics: the device stages (all-pairs Hellinger, knn_membership, the layout on the LDS path and on the per-epoch
path), the host steps between them, and the NumPy restatement of tests/test_device_embedding.py for the same inputs.

    python tools/embedding_timing.py [--reps 3] [--no-numpy]

Every device time is a host clock around a call that ends in a stream synchronise; the first call of each kind is a warm-up
and is not reported.  Needs a real MI355X."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def best(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return min(times), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-numpy", action="store_true")
    args = ap.parse_args()
    from enstop_amd import embedding
    from enstop_amd.engine import Engine
    import test_device_embedding as restated
    a, b = embedding.find_ab_params()
    with Engine() as eng:
        print(eng.device_info())
        for starts, topics in ((16, 10), (32, 20), (128, 20)):
            t = starts * topics
            base = np.random.RandomState(0).dirichlet(np.full(2000, 0.05), size=topics)
            stack = restated.stack_of(base, starts, 200.0, seed=1)
            ms = {}
            ms["hellinger"], D = best(lambda: eng.all_pairs_hellinger(stack), args.reps)
            ms["knn_membership"], knn = best(lambda: eng.knn_membership(D, 15), args.reps)

            def host():
                W = embedding.prune_for_schedule(embedding.fuzzy_graph(knn[0], knn[4]), 500)
                return (W,) + embedding.initial_layout(W, 5, 0)
            ms["host graph+init"], (W, Y0, init, components) = best(host, args.reps)
            fits = 2 * t * 5 * 4 <= 65536
            if fits:
                ms["layout lds"], Y = best(lambda: eng.layout(W, Y0, n_epochs=500, a=a, b=b, path="lds"), args.reps)
            ms["layout epoch"], Y2 = best(lambda: eng.layout(W, Y0, n_epochs=500, a=a, b=b, path="epoch"), args.reps)
            assert not fits or np.array_equal(Y, Y2)
            ms["whole stage"], _ = best(lambda: eng.hellinger_embedding(stack), args.reps)
            if not args.no_numpy:
                t0 = time.perf_counter()
                restated.knn_restated(D, 15)
                ms["numpy knn"] = time.perf_counter() - t0
                t0 = time.perf_counter()
                restated.layout_restated(W, Y0, 500, a, b, dtype=np.float32)
                ms["numpy layout"] = time.perf_counter() - t0
            print("t=%d  init=%s components=%d edges=%d  " % (t, init, components, W.nnz)
                  + "  ".join("%s %.2f ms" % (k, 1e3 * v) for k, v in ms.items())
                  + ("" if fits else "  (layout lds: does not fit 64 KiB)"), flush=True)


if __name__ == "__main__":
    main()

"""Bits of the topic combination, for comparing two builds of the library: runs the six entry points of csrc/plsa_combine.hpp on
fixed seeded inputs and writes, per case, the SHA-256 of each output array's bytes as one JSON object.

    ENSTOP_AMD_LIB=/path/to/libplsa_hip.so python tools/combine_ab.py --out a.json
    python tools/combine_ab.py --out b.json
    python tools/combine_ab.py --compare a.json b.json        (exit status 1 and the differing cases when they differ)

The cases are the smallest at which each piece can go wrong: one tile and several (t = 64, 65, 130, 200), one word, a ragged last
slice (m = 33, 4037), a row of zeros, a subnormal entry; representatives around one workgroup of words (m = 255, 257) with
noise and an empty cluster, with and without weights; co-document counts in one pass and in passes of 3 sets; k-NN with t
below, above and far above a wavefront; the layout on both paths.  Every run is a process of its own.  Needs a real MI355X."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sha(*arrays):
    return [hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() for a in arrays]


def topics_of(t, m, seed, variant):
    T = np.random.RandomState(seed).dirichlet(np.full(m, 0.3), size=t).astype(np.float32)
    if variant == "zero_row":
        T[t // 2] = 0.0
    if variant == "subnormal":
        T[t - 1, m // 2] = np.float32(3e-41)
    return T


def run():
    import scipy.sparse as sp
    from enstop_amd import embedding
    from enstop_amd.engine import Engine
    out = {}
    with Engine() as eng:
        for t in (1, 64, 65, 130, 200):
            for m in (1, 33, 4037):
                for variant in ("plain", "zero_row", "subnormal"):
                    T = topics_of(t, m, 1000 * t + m, variant)
                    out["pairs t=%d m=%d %s" % (t, m, variant)] = sha(eng.all_pairs_hellinger(T), eng.all_pairs_kl(T))
        for m in (255, 257):
            T = topics_of(40, m, m, "plain")
            labels = np.random.RandomState(7).randint(-1, 6, size=40)
            labels[labels == 3] = 4                       # cluster 3 is empty
            w = np.random.RandomState(8).rand(40)
            out["representatives m=%d" % m] = sha(eng.cluster_representatives(T, labels),
                                                  eng.cluster_representatives(T, labels, w))
        X = sp.random(5000, 300, density=0.03, format="csr", dtype=np.float32, random_state=np.random.RandomState(3))
        X.data[::5] = 0.0                                 # stored entries that are not positive
        eng.upload_csr(X)
        words = np.stack([np.random.RandomState(20 + s).choice(300, size=4, replace=False) for s in range(7)])
        for cap in (0, 3):
            out["codocument cap=%d" % cap] = sha(*eng.codocument_counts(words, max_sets_per_pass=cap))
        a, b = embedding.find_ab_params()
        for t in (2, 65, 300):
            D = np.random.RandomState(t).rand(t, t)
            D = D + D.T
            np.fill_diagonal(D, 0.0)
            for k in (1, 15):
                knn = eng.knn_membership(D, k)
                out["knn t=%d k=%d" % (t, k)] = sha(*knn)
        W = embedding.fuzzy_graph(knn[0], knn[4])             # t = 300, 15 neighbours
        for dim in (2, 5):
            Y0 = np.random.RandomState(dim).uniform(-10, 10, size=(300, dim)).astype(np.float32)
            for path in ("lds", "epoch"):
                out["layout dim=%d %s" % (dim, path)] = sha(eng.layout(W, Y0, n_epochs=20, a=a, b=b, seed=5, path=path))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    if args.compare:
        one, other = (json.load(open(p)) for p in args.compare)
        differ = sorted(k for k in set(one) | set(other) if one.get(k) != other.get(k))
        print(json.dumps(dict(cases=len(one), equal=not differ, differ=differ)))
        return 1 if differ else 0
    result = run()
    text = json.dumps(result, indent=1, sort_keys=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print("%d cases, digest of all: %s" % (len(result), hashlib.sha256(text.encode()).hexdigest()))
    return 0


if __name__ == "__main__":
    sys.exit(main())

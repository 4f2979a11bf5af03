"""The native embedding behind topic_combination="hellinger_umap" (include/plsa_hip_embed.h, csrc/plsa_embed_kernels.hpp)
against a NumPy float64 restatement of UMAP as published, written below step by step.  Needs a real MI355X (-m gpu).

The restatement (none of it calls enstop_amd/embedding.py):

    knn_restated       steps 1-3: stable argsort, rho, the 64-step bisection for sigma with its floors, memberships
    graph_restated     steps 4-5: W = A + A^T - A o A^T, entries below max(W) / n_epochs dropped
    init_restated      step 7: normalised-Laplacian eigenvectors (dense eigh) or seeded uniform positions
    layout_restated    step 8: the synchronous layout, in float64 or (dtype=np.float32) in float32

What is float32 BY DEFINITION on both sides: the neighbour distances handed on (float32 of D's entries), a and b, the
initial positions, and the sampling schedule (epochs per sample max(W) / w, the per-edge epochs of the next sample and of
the next negative sample, the number of negative samples int((n - next) / per_negative)).  The schedule is discrete -- a
rounding difference there is a different set of edges, not a small error -- so its float32 operations are restated
operation for operation and only positions and gradients are float64 in the float64 restatement.  The negative-sample
vertex is (splitmix64 finaliser of (seed, epoch, edge, sample) >> 32) mod t.

Tolerances.
  neighbours   idx, dist, rho exact.  sigma rtol 1e-4: each side stops its bisection within 1e-5 of log2(k) on a sum whose
               derivative in log(sigma) is of order 1, and a float32 sum of <= 199 terms of <= 1 is good to a few 1e-6.
               member atol 1e-5 likewise (a membership is one term of that sum).
  one epoch    atol 1e-3: a vertex sums at most about 6 * deg ~ 240 clipped terms of magnitude <= 4, each good to a few
               float32 ulp (2.4e-7 * 4 * 240 * a few ~ 1e-3); a wrong edge, a missing factor 2, a wrong alpha or a wrong
               sample count moves a vertex by >= 1e-2.  Epoch 0 of the schedule samples nothing (an edge is first due in
               epoch max(W) / w >= 1, as in umap-learn), so "one epoch" is n_epochs = 2: epoch 1 is the one that acts.
  ten epochs   MEASURED, not chosen: 8 x the largest deviation of the float32 restatement from the float64 one on the same
               inputs (rounding differences between powf implementations compound through the repulsive term's steep
               region; a structural error is orders of magnitude above).  Printed by the test; DESIGN.md section 13.
               Five dimensions only: on these random graphs in TWO dimensions vertices pass through each other within
               ten epochs, the clipped repulsion changes sign with the last bit, and the float32 restatement itself ends
               3 to 5 units from the float64 one (t = 65 and 300, two seeds each) -- a bound that bounds nothing.  In five
               dimensions it stays at 1e-4 ... 2e-4.
  same bits    the LDS path and the per-epoch path: array_equal.
"""
import numpy as np
import pytest
import scipy.sparse as sp

GOLDEN = np.uint64(0x9E3779B97F4A7C15)


# ------------------------------------------------------------------------------------------------------------------
# the restatement

def knn_restated(D, k):
    D = np.asarray(D, np.float64)
    t = D.shape[0]
    idx = np.argsort(D, axis=1, kind="stable")[:, :k]
    dist = np.take_along_axis(D, idx, axis=1).astype(np.float32)
    d = dist.astype(np.float64)
    rho, sigma, member = np.zeros(t), np.zeros(t), np.zeros((t, k))
    target = np.log2(k)
    for i in range(t):
        row = d[i]
        r = row[row > 0].min() if (row > 0).any() else 0.0
        x = row - r
        lo, hi, mid = 0.0, np.inf, 1.0
        for _ in range(64):
            with np.errstate(over="ignore", divide="ignore"):
                psum = np.where(x[1:] > 0, np.exp(-(x[1:] / mid)), 1.0).sum()
            if abs(psum - target) < 1e-5:
                break
            if psum > target:
                hi = mid
                mid = (lo + hi) / 2.0
            else:
                lo = mid
                mid = mid * 2.0 if hi == np.inf else (lo + hi) / 2.0
        mid = max(mid, 1e-3 * (row.mean() if r > 0 else d.mean()))
        rho[i], sigma[i] = r, mid
        with np.errstate(over="ignore"):
            member[i] = np.where(idx[i] == i, 0.0, np.where(x > 0, np.exp(-(x / mid)), 1.0))
    return idx, dist, rho, sigma, member


def graph_restated(idx, member, n_epochs):
    t, k = idx.shape
    A = np.zeros((t, t))
    A[np.repeat(np.arange(t), k), idx.ravel()] = np.asarray(member, np.float64).ravel()
    W = A + A.T - A * A.T
    W[W < W.max() / float(n_epochs)] = 0.0
    return sp.csr_matrix(W)


def init_restated(W, dim, seed):
    A = np.asarray(W.todense())
    t = A.shape[0]
    rng = np.random.RandomState(seed)
    deg = A.sum(axis=1)
    s = np.zeros(t)
    s[deg > 0] = deg[deg > 0] ** -0.5
    L = np.diag((deg > 0) * 1.0) - s[:, None] * A * s[None, :]
    vals, vecs = np.linalg.eigh((L + L.T) / 2.0)
    components = int((vals < 1e-8).sum())
    if components > 1 or t <= dim + 1:
        return rng.uniform(0.0, 10.0, size=(t, dim)).astype(np.float32), "random", components
    Y = vecs[:, 1:dim + 1].copy()
    for c in range(dim):
        if Y[np.abs(Y[:, c]).argmax(), c] < 0:
            Y[:, c] = -Y[:, c]
    Y *= 10.0 / np.abs(Y).max()
    Y += rng.normal(scale=1e-4, size=Y.shape)
    Y = 10.0 * (Y - Y.min(axis=0)) / (Y.max(axis=0) - Y.min(axis=0))
    return Y.astype(np.float32), "spectral", components


def mix64(x):
    x = np.array(x, dtype=np.uint64, ndmin=1)
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return x


def layout_restated(W, Y0, n_epochs, a, b, rate=5, seed=0, dtype=np.float64):
    W = sp.csr_matrix(W)
    W.sort_indices()
    t = W.shape[0]
    indptr, indices = W.indptr, W.indices.astype(np.int64)
    src = np.repeat(np.arange(t), np.diff(indptr))
    w = W.data.astype(np.float32)
    f32 = np.float32
    eps = (w.max() / w).astype(f32) if w.size else w            # the schedule: float32, operation for operation
    epn = (eps / f32(rate)).astype(f32)
    next_sample, next_negative = eps.copy(), epn.copy()
    a_, b_ = dtype(f32(a)), dtype(f32(b))
    two_ab, two_b, tiny = dtype(2) * a_ * b_, dtype(2) * b_, dtype(f32(0.001))
    one, four = dtype(1), dtype(4)
    Y = np.asarray(Y0, f32).astype(dtype)

    def coefficient(diff, live, attractive):
        d2 = (diff * diff).sum(axis=1, dtype=dtype)
        c = np.zeros(len(d2), dtype)
        m = live & (d2 > 0)
        pb = d2[m] ** b_
        c[m] = -(two_ab * pb) / (d2[m] * (a_ * pb + one)) if attractive else two_b / ((tiny + d2[m]) * (a_ * pb + one))
        return np.clip(c[:, None] * diff, -four, four)

    for epoch in range(n_epochs):
        fn = f32(epoch)
        alpha = dtype(f32(1) - fn / f32(n_epochs))
        G = np.zeros_like(Y)
        e = np.flatnonzero(next_sample <= fn)
        i, j = src[e], indices[e]
        np.add.at(G, i, dtype(2) * coefficient(Y[i] - Y[j], np.ones(len(e), bool), True))
        next_sample[e] += eps[e]
        n_neg = np.trunc((fn - next_negative[e]) / epn[e]).astype(np.int64)
        with np.errstate(over="ignore"):
            key = mix64(np.uint64(seed) + GOLDEN * np.uint64(epoch + 1))
            ekey = mix64(key ^ e.astype(np.uint64))
            for p in range(int(n_neg.max()) if e.size else 0):
                sel = n_neg > p
                h = mix64(ekey[sel] + GOLDEN * np.uint64(p + 1))
                v = ((h >> np.uint64(32)) % np.uint64(t)).astype(np.int64)
                np.add.at(G, i[sel], coefficient(Y[i[sel]] - Y[v], v != i[sel], False))
        next_negative[e] += n_neg.astype(f32) * epn[e]
        Y = Y + alpha * G
    return Y


def embedding_restated(D, n_neighbors=15, dim=5, seed=0, n_epochs=500, ab=(1.5769434, 0.8950609), dtype=np.float64):
    idx, _, _, _, member = knn_restated(D, min(n_neighbors, D.shape[0] - 1))
    W = graph_restated(idx, member.astype(np.float32), n_epochs)
    Y0, init, components = init_restated(W, dim, seed)
    return layout_restated(W, Y0, n_epochs, ab[0], ab[1], seed=seed, dtype=dtype), init, components


# ------------------------------------------------------------------------------------------------------------------
# inputs

def euclidean(P):
    P = np.asarray(P, np.float64)
    return np.sqrt(((P[:, None, :] - P[None, :, :]) ** 2).sum(axis=-1))


def distance_case(t, kind):
    rs = np.random.RandomState(1000 + t)
    if kind == "generic":
        P = rs.rand(t, 3)
    elif kind == "lattice":                      # integer coordinates: many exactly tied distances, duplicated points
        P = rs.randint(0, 3, size=(t, 2)).astype(np.float64)
    else:                                        # "clone": min(t - 1, 16) copies of one point -> rows with rho = 0 at k <= that
        P = rs.rand(t, 3)
        P[:min(t - 1, 16)] = P[0]
    return euclidean(P)


def random_graph(t, deg, seed, isolated=None, equal_weights=False):
    rs = np.random.RandomState(seed)
    A = np.zeros((t, t))
    for i in range(t):
        nb = rs.choice(t, size=min(deg, t - 1), replace=False)
        A[i, nb[nb != i]] = 1.0 if equal_weights else rs.choice([1.0, 0.5, 0.31, 0.07], size=(nb != i).sum())
    W = np.maximum(A, A.T)
    if isolated is not None:
        W[isolated, :] = 0.0
        W[:, isolated] = 0.0
    return sp.csr_matrix(W)


def stack_of(base, starts, scale, seed):
    rs = np.random.RandomState(seed)
    return np.vstack([rs.dirichlet(scale * b + 1e-3, size=starts) for b in base]).astype(np.float32)


AB = (1.5769434, 0.8950609)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from enstop_amd.engine import Engine
    with Engine() as e:
        yield e


# ------------------------------------------------------------------------------------------------------------------
# steps 1-3

KNN_CASES = [(t, k, kind) for t in (2, 17, 64, 65, 200) for k in sorted({1, min(15, t - 1), t - 1})
             for kind in ("generic", "lattice", "clone")]


@pytest.mark.parametrize("t,k,kind", KNN_CASES)
def test_neighbours_bandwidths_and_memberships(eng, t, k, kind):
    D = distance_case(t, kind)
    idx, dist, rho, sigma, member = eng.knn_membership(D, k)
    want = knn_restated(D, k)
    assert idx.dtype == np.int32 and idx.shape == (t, k)
    np.testing.assert_array_equal(idx, want[0])
    np.testing.assert_array_equal(dist, want[1])
    np.testing.assert_array_equal(rho, want[2].astype(np.float32))
    if kind == "clone" and k <= min(t - 1, 16):
        assert (rho[:min(t - 1, 16)] == 0).all()                     # every neighbour of a clone is at distance 0
    np.testing.assert_allclose(sigma, want[3], rtol=1e-4)
    np.testing.assert_allclose(member, want[4], rtol=0, atol=1e-5)


def test_neighbour_arguments(eng):
    from enstop_amd.engine import DeviceError
    with pytest.raises(ValueError):
        eng.knn_membership(np.zeros((1, 1)), 15)
    D = distance_case(17, "generic")
    assert eng.knn_membership(D, 100)[0].shape == (17, 16)           # capped at t - 1
    D[3, 4] = np.nan
    with pytest.raises(DeviceError, match="finite"):
        eng.knn_membership(D, 5)


# ------------------------------------------------------------------------------------------------------------------
# step 8

def layout_inputs(t, dim, seed=0):
    """(W, Y0, isolated vertex or None).  t = 3: a triangle of equal weights whose vertices 1 and 2 coincide; otherwise
    15 random neighbours per vertex with weights from {1, 0.5, 0.31, 0.07}, the last vertex isolated, and a neighbour of
    vertex 0 at vertex 0's position (d^2 = 0 on an edge)."""
    Y0 = np.random.RandomState(seed + 1).uniform(0, 10, size=(t, dim)).astype(np.float32)
    if t == 3:
        Y0[2] = Y0[1]
        return sp.csr_matrix(np.ones((3, 3)) - np.eye(3)), Y0, None
    W = random_graph(t, 15, seed, isolated=t - 1)
    Y0[W.indices[W.indptr[0]]] = Y0[0]
    return W, Y0, t - 1


def assert_within_measured_bound(got, W, Y0, n_epochs, seed):
    want = layout_restated(W, Y0, n_epochs, AB[0], AB[1], seed=seed)
    f32 = layout_restated(W, Y0, n_epochs, AB[0], AB[1], seed=seed, dtype=np.float32)
    measured = float(np.abs(f32.astype(np.float64) - want).max())
    print("t=%d dim=%d, %d epochs: float32 restatement off float64 by %.3g, bound %.3g, device off by %.3g"
          % (Y0.shape + (n_epochs, measured, 8.0 * measured, np.abs(got - want).max())))
    assert 0 < measured < 1e-2                                       # far below a structural error
    np.testing.assert_allclose(got, want, rtol=0, atol=8.0 * measured)


@pytest.mark.parametrize("dim", [2, 5])
@pytest.mark.parametrize("t", [3, 65, 300])
@pytest.mark.parametrize("path", [1, 2])
def test_one_epoch_of_layout(eng, t, dim, path):
    W, Y0, isolated = layout_inputs(t, dim)
    got = eng.layout(W, Y0, n_epochs=2, a=AB[0], b=AB[1], seed=7, path=path)
    want = layout_restated(W, Y0, 2, AB[0], AB[1], seed=7)
    moved = np.abs(want - Y0).max(axis=1)
    print("t=%d dim=%d path=%d: max |got - want| = %.3g, vertices moved %d, largest move %.3g"
          % (t, dim, path, np.abs(got - want).max(), (moved > 0).sum(), moved.max()))
    assert (moved > 1e-2).sum() >= t // 2                            # the epoch acts: the comparison is not of two copies
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-3)
    if isolated is not None:
        np.testing.assert_array_equal(got[isolated], Y0[isolated])   # the isolated vertex does not move at all


@pytest.mark.parametrize("t,dim", [(65, 5), (300, 5)])
def test_ten_epochs_against_float64(eng, t, dim):
    W, Y0, _ = layout_inputs(t, dim, seed=3)
    assert_within_measured_bound(eng.layout(W, Y0, n_epochs=10, a=AB[0], b=AB[1], seed=11), W, Y0, 10, 11)


def test_both_paths_give_the_same_bits_over_a_whole_layout(eng):
    W, Y0, _ = layout_inputs(300, 5, seed=5)
    lds = eng.layout(W, Y0, seed=2, path=1)
    assert eng.last_layout_path == "lds"
    per_epoch = eng.layout(W, Y0, seed=2, path=2)
    assert eng.last_layout_path == "epoch"
    assert np.isfinite(lds).all() and np.abs(lds - Y0).max() > 0.1
    np.testing.assert_array_equal(lds.view(np.uint32), per_epoch.view(np.uint32))
    np.testing.assert_array_equal(eng.layout(W, Y0, seed=2, path=1).view(np.uint32), lds.view(np.uint32))      # one seed, two runs
    assert not np.array_equal(eng.layout(W, Y0, seed=3, path=1), lds)                                        # two seeds


def test_the_lds_limit(eng):
    """2 * t * 5 * 4 bytes: 65 520 at t = 1638 (fits 64 KiB), 65 560 at t = 1639 (does not)."""
    from enstop_amd.engine import DeviceError
    W, Y0, _ = layout_inputs(1638, 5, seed=8)
    kw = dict(n_epochs=3, a=AB[0], b=AB[1], seed=4)
    auto = eng.layout(W, Y0, **kw)
    assert eng.last_layout_path == "lds"
    np.testing.assert_array_equal(auto.view(np.uint32), eng.layout(W, Y0, path=2, **kw).view(np.uint32))
    np.testing.assert_array_equal(auto.view(np.uint32), eng.layout(W, Y0, path=1, **kw).view(np.uint32))
    assert_within_measured_bound(auto, W, Y0, 3, 4)
    W, Y0, _ = layout_inputs(1639, 5, seed=9)
    auto = eng.layout(W, Y0, **kw)
    assert eng.last_layout_path == "epoch"
    np.testing.assert_array_equal(auto.view(np.uint32), eng.layout(W, Y0, path=2, **kw).view(np.uint32))
    assert_within_measured_bound(auto, W, Y0, 3, 4)
    with pytest.raises(DeviceError, match="LDS"):
        eng.layout(W, Y0, path=1, **kw)


# ------------------------------------------------------------------------------------------------------------------
# the whole stage, by properties

def nearest_base(stable, base):
    """index of the base topic nearest in Hellinger distance to every stable topic"""
    bc = np.sqrt(np.asarray(stable, np.float64)) @ np.sqrt(np.asarray(base, np.float64)).T
    return np.sqrt(np.clip(1.0 - bc, 0.0, None)).argmin(axis=1)


def test_clean_ensemble_embeds_and_combines(eng):
    from sklearn.manifold import trustworthiness
    from enstop_amd import ensemble
    base = np.random.RandomState(0).dirichlet(np.full(2000, 0.05), size=10)
    stack = stack_of(base, 16, 200.0, seed=1)
    Y = eng.hellinger_embedding(stack, n_neighbors=15, n_components=5, seed=0)
    info = eng.last_embedding_info
    print(info)
    assert Y.shape == (160, 5) and Y.dtype == np.float32 and np.isfinite(Y).all()
    assert info["init"] == "random" and info["components"] == 10 and info["t"] == 160 and info["n_neighbors"] == 15
    assert info["n_epochs"] == 500 and info["path"] == "lds" and info["edges"] > 0
    tw = trustworthiness(eng.all_pairs_hellinger(stack), Y, n_neighbors=15, metric="precomputed")
    print("trustworthiness %.4f" % tw)
    assert tw > 0.95
    stable = ensemble.generate_combined_topics_hellinger_umap(stack, engine=eng)
    assert stable.shape == (10, 2000)
    assert sorted(nearest_base(stable, base).tolist()) == list(range(10))


def test_overlapping_ensemble_starts_from_the_spectral_layout(eng):
    from sklearn.manifold import trustworthiness
    base = np.random.RandomState(0).dirichlet(np.full(1000, 0.05), size=10)
    stack = stack_of(base, 12, 5.0, seed=1)
    Y = eng.hellinger_embedding(stack, n_neighbors=15, n_components=5, seed=0)
    info = eng.last_embedding_info
    print(info)
    assert info["init"] == "spectral" and info["components"] == 1 and np.isfinite(Y).all()
    tw = trustworthiness(eng.all_pairs_hellinger(stack), Y, n_neighbors=15, metric="precomputed")
    print("trustworthiness %.4f" % tw)
    assert tw > 0.85

"""CPU-only checks of the embedding boundary (include/plsa_hip_embed.h): the header declares exactly plsa_knn_membership and
plsa_layout, it is plain C99, the built library exports them, enstop_amd/_lib.py binds them in a table of its own,
INTEGRATION.md documents them, and the other headers and tables are untouched by them.  Plus the host steps that lie
between the two entry points (enstop_amd/embedding.py): the curve parameters, the fuzzy graph, the initial layout.
No device computation here."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT

HEADER = "plsa_hip_embed.h"
NAMES = ["plsa_knn_membership", "plsa_layout"]
OTHER_HEADERS = ("plsa_hip.h", "plsa_hip_diag.h", "plsa_hip_members.h", "plsa_hip_metrics.h", "plsa_hip_blocked.h")


def _symbols(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(plsa_[a-z0-9_]+)\s*\(", text)))


def _arguments(header, name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
    return [" ".join(a.split()) for a in args.split(",")]


def test_embed_header_declares_exactly_the_two_entry_points():
    assert _symbols(HEADER) == NAMES


def test_embed_header_is_plain_c99():
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c",
                          os.path.join(ROOT, "include", HEADER)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_embed_symbols_exported_and_bound_in_their_own_table():
    from enstop_amd import _lib
    lib = _lib.load()
    assert sorted(_lib.EMBED_SIGNATURES) == NAMES
    for name, (res, args) in _lib.EMBED_SIGNATURES.items():
        assert hasattr(lib, name), "libplsa_hip.so does not export %s" % name
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype == res            # applied by load()


def test_embed_signatures_match_the_header():
    """argument for argument: the C type of the header against the ctypes type of the table"""
    import ctypes as C
    from enstop_amd import _lib
    kinds = {"plsa_ctx *": [C.c_void_p], "int64_t": [C.c_int64], "int32_t": [C.c_int32], "uint64_t": [C.c_uint64], "float": [C.c_float],
             "const double *": [_lib._f64p], "const int32_t *": [_lib._i32p], "int32_t *": [_lib._i32p],
             "const float *": [_lib._f32p], "float *": [_lib._f32p]}
    for name in NAMES:
        res, args = _lib.EMBED_SIGNATURES[name]
        declared = _arguments(HEADER, name)
        assert res is C.c_int and len(declared) == len(args), name
        for text, ctype in zip(declared, args):
            c_type = re.sub(r"\s*\b\w+$", "", text).strip()                # drop the parameter's name
            assert c_type in kinds and ctype in kinds[c_type], (name, text, ctype)


def test_embed_symbols_stay_out_of_the_other_headers_and_tables():
    from enstop_amd import _lib
    names = set(NAMES)
    for other in OTHER_HEADERS:
        assert not names & set(_symbols(other)), other
    for table in (_lib.SIGNATURES, _lib.MEMBER_SIGNATURES, _lib.METRIC_SIGNATURES, _lib.BLOCKED_SIGNATURES):
        assert not names & set(table)
    assert sorted(_lib.SIGNATURES) == sorted(set(_symbols("plsa_hip.h")) | set(_symbols("plsa_hip_diag.h")))


def test_embed_entry_points_are_documented_with_the_interface_they_stand_for():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(n in doc for n in NAMES) and HEADER in doc and "enstop_.py:354-414" in doc
    header = open(os.path.join(ROOT, "include", HEADER)).read()
    assert header.count("enstop_.py:354-414") >= 3                  # the file's head and each entry


def test_curve_parameters():
    from enstop_amd import embedding
    a, b = embedding.find_ab_params()
    assert abs(a - 1.577) < 1e-3 and abs(b - 0.895) < 1e-3, (a, b)
    assert embedding.default_n_epochs(10000) == 500 and embedding.default_n_epochs(10001) == 200


def _memberships(t, k, seed):
    rs = np.random.RandomState(seed)
    idx = np.stack([np.concatenate([[i], rs.choice(np.delete(np.arange(t), i), k - 1, replace=False)]) for i in range(t)])
    member = rs.rand(t, k).astype(np.float32)
    member[:, 0] = 0.0
    return idx.astype(np.int32), member


def test_fuzzy_graph_is_the_probabilistic_union():
    from enstop_amd import embedding
    idx, member = _memberships(40, 6, 0)
    A = np.zeros((40, 40))
    A[np.repeat(np.arange(40), 6), idx.ravel()] = member.ravel()
    want = A + A.T - A * A.T
    W = embedding.fuzzy_graph(idx, member)
    assert W.has_sorted_indices and (W.data > 0).all()
    np.testing.assert_allclose(W.toarray(), want, rtol=1e-15, atol=0)
    pruned = embedding.prune_for_schedule(W, 20)
    want[want < want.max() / 20.0] = 0.0
    assert 0 < pruned.nnz < W.nnz
    np.testing.assert_allclose(pruned.toarray(), want, rtol=1e-15, atol=0)


def test_initial_layout_spectral_and_random():
    from enstop_amd import embedding
    idx, member = _memberships(60, 8, 1)
    W = embedding.fuzzy_graph(idx, member)
    Y, kind, components = embedding.initial_layout(W, 3, seed=5)
    assert kind == "spectral" and components == 1 and Y.shape == (60, 3) and Y.dtype == np.float32
    np.testing.assert_allclose(Y.min(axis=0), 0.0, atol=1e-6)
    np.testing.assert_allclose(Y.max(axis=0), 10.0, atol=1e-5)
    # the coordinates are eigenvectors 1..3 of the normalised Laplacian, up to the affine rescaling and the 1e-4 noise
    A = W.toarray()
    s = A.sum(axis=1) ** -0.5
    vecs = np.linalg.eigh(np.eye(60) - s[:, None] * A * s[None, :])[1][:, 1:4]
    for c in range(3):
        assert abs(np.corrcoef(Y[:, c], vecs[:, c])[0, 1]) > 1 - 1e-6
        assert Y[np.abs(vecs[:, c]).argmax(), c] == Y[:, c].max()     # signed so that the largest-magnitude entry is positive
    np.testing.assert_array_equal(Y, embedding.initial_layout(W, 3, seed=5)[0])
    assert not np.array_equal(Y, embedding.initial_layout(W, 3, seed=6)[0])
    # two components (a block-diagonal graph) and an isolated vertex: seeded uniform positions
    two = sp.block_diag([W, W]).tocsr()
    Y2, kind2, components2 = embedding.initial_layout(two, 3, seed=5)
    assert kind2 == "random" and components2 == 2 and Y2.shape == (120, 3) and Y2.min() >= 0 and Y2.max() <= 10
    lone = sp.block_diag([W, sp.csr_matrix((1, 1))]).tocsr()
    assert embedding.initial_layout(lone, 3, seed=5)[1:] == ("random", 2)


def test_combiner_environment_switch(monkeypatch):
    from enstop_amd import ensemble
    monkeypatch.setenv("ENSTOP_AMD_EMBEDDING", "sometimes")
    with pytest.raises(ValueError, match="ENSTOP_AMD_EMBEDDING"):
        ensemble.generate_combined_topics_hellinger_umap(np.ones((8, 4)) / 4)

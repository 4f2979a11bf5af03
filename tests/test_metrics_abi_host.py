"""CPU-only checks of the device-metrics boundary (include/plsa_hip_metrics.h): the header declares exactly
plsa_codocument_counts, the built library exports it, enstop_amd/_lib.py binds it in a table of its own, INTEGRATION.md
documents it, and the two drop-in headers and their table are untouched by it.  Plus the host half of the coherence split:
_coherence_from_counts on counts from a dense B.T @ B equals utils.coherence(backend="host"), float64 bit for bit.
No device computation here."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT, golden_csr, load_golden

HEADER = "plsa_hip_metrics.h"


def _symbols(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(plsa_[a-z0-9_]+)\s*\(", text)))


def test_metric_header_declares_exactly_the_one_entry_point():
    assert _symbols(HEADER) == ["plsa_codocument_counts"]


def test_metric_symbol_exported_and_bound_in_its_own_table():
    from enstop_amd import _lib
    lib = _lib.load()
    assert sorted(_lib.METRIC_SIGNATURES) == _symbols(HEADER)
    for name, (res, args) in _lib.METRIC_SIGNATURES.items():
        assert hasattr(lib, name), "libplsa_hip.so does not export %s" % name
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype == res            # applied by load()
    assert len(_lib.METRIC_SIGNATURES["plsa_codocument_counts"][1]) == 7


def test_metric_symbol_stays_out_of_the_existing_headers_and_tables():
    from enstop_amd import _lib
    names = set(_symbols(HEADER))
    for other in ("plsa_hip.h", "plsa_hip_diag.h", "plsa_hip_members.h"):
        assert not names & set(_symbols(other)), other
    assert not names & set(_lib.SIGNATURES) and not names & set(_lib.MEMBER_SIGNATURES)
    assert sorted(_lib.SIGNATURES) == sorted(set(_symbols("plsa_hip.h")) | set(_symbols("plsa_hip_diag.h")))


def test_metric_entry_point_is_documented_with_the_interface_it_stands_for():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "plsa_codocument_counts" in doc and HEADER in doc and "enstop/utils.py:150-203" in doc


def test_metric_header_is_plain_c():
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c",
                          os.path.join(ROOT, "include", HEADER)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def _dense_counts(X, top):
    """co-document counts and positive-entry counts of the word list `top`, from a dense stored-entry pattern"""
    X = sp.csr_matrix(X)
    B = np.zeros(X.shape, np.int64)
    B[np.repeat(np.arange(X.shape[0]), np.diff(X.indptr)), X.indices] = 1          # stored entries, zeros included
    positive = np.zeros(X.shape, np.int64)
    positive[np.repeat(np.arange(X.shape[0]), np.diff(X.indptr)), X.indices] = X.data > 0
    return B[:, top].T @ B[:, top], positive[:, top].sum(axis=0)


def _corpus_with_stored_zeros():
    rs = np.random.RandomState(11)
    X = sp.random(300, 97, density=0.08, format="csr", random_state=rs, data_rvs=lambda size: rs.randint(1, 5, size).astype(np.float64))
    X.data[rs.rand(X.nnz) < 0.1] = 0.0                  # stored zeros: in the pattern, not in `data > 0`
    col = X.tocsc()
    assert col.indptr[6] - col.indptr[5] > 0
    X.data[X.indices == 5] = 0.0                        # one column of stored zeros only
    assert (X.data == 0).sum() > 20 and X.has_canonical_format
    T = rs.rand(4, 97)
    T[:, 5] += 2.0                                      # ... which every topic ranks first
    return X, T


@pytest.mark.parametrize("case", ["golden", "stored_zeros"])
def test_coherence_from_counts_equals_the_host_path(case):
    from enstop_amd import utils
    if case == "golden":
        g = load_golden("metrics")
        X, T, n_words = golden_csr(g), g["topics"], 10
    else:
        X, T = _corpus_with_stored_zeros()
        n_words = 20
    per_topic = []
    for z in range(T.shape[0]):
        top = np.argsort(T[z])[-n_words:]
        co, positive = _dense_counts(X, top)
        if case == "stored_zeros":
            assert positive[-1] == 0 and co[-1, -1] > 0          # the all-zero column is the last (highest) word
        got = utils._coherence_from_counts(co, positive)
        want = utils.coherence(T, z, X, n_words=n_words, backend="host")
        assert isinstance(got, float) and got == want, (z, got, want)
        per_topic.append(got)
    assert np.mean(per_topic) == utils.mean_coherence(T, X, n_words=n_words, backend="host")
    if case == "golden":
        np.testing.assert_allclose(per_topic, g["coherence"], rtol=1e-10)


def test_host_backend_is_selectable_and_reported(monkeypatch):
    from enstop_amd import utils
    X, T = _corpus_with_stored_zeros()
    monkeypatch.delenv("ENSTOP_AMD_METRICS", raising=False)
    utils.last_metric_path = None
    a = utils.mean_coherence(T, X, n_words=5, backend="host")
    assert utils.last_metric_path == "host"
    utils.last_metric_path = None
    assert utils.coherence(T, 1, X, n_words=5, backend="host") == utils.coherence(T, 1, X, n_words=5, backend="host")
    assert utils.last_metric_path == "host"
    monkeypatch.setenv("ENSTOP_AMD_METRICS", "host")
    utils.last_metric_path = None
    assert utils.mean_coherence(T, X, n_words=5) == a
    assert utils.last_metric_path == "host"
    monkeypatch.setenv("ENSTOP_AMD_METRICS", "sometimes")
    with pytest.raises(ValueError, match="ENSTOP_AMD_METRICS"):
        utils.mean_coherence(T, X, n_words=5)
    with pytest.raises(ValueError, match="backend"):
        utils.mean_coherence(T, X, n_words=5, backend="gpu")


def test_calls_the_device_cannot_carry_run_on_the_host_unless_it_was_demanded(monkeypatch):
    """n_words > 32, dense data and a non-canonical matrix: host under backend=None whatever the environment selects,
    ValueError (raised before any device is looked for) under backend="device"."""
    from enstop_amd import utils
    X, T = _corpus_with_stored_zeros()

    def cases():          # (fresh every time: SciPy sums the duplicates of a matrix in place when it is compared)
        dup = sp.csr_matrix((np.ones(4), np.array([1, 1, 0, 2]), np.array([0, 2, 4])), shape=(2, 97))     # a duplicate entry
        assert not dup.has_canonical_format
        return [(T, X, 40), (T, X.toarray(), 5), (T, dup, 3)]

    for env in ("auto", "device"):
        monkeypatch.setenv("ENSTOP_AMD_METRICS", env)
        for topics, data, n_words in cases():
            utils.last_metric_path = None
            utils.mean_coherence(topics, data, n_words=n_words)
            assert utils.last_metric_path == "host"
    for topics, data, n_words in cases():
        with pytest.raises(ValueError, match="device"):
            utils.mean_coherence(topics, data, n_words=n_words, backend="device")
        with pytest.raises(ValueError, match="device"):
            utils.coherence(topics, 0, data, n_words=n_words, backend="device")
    assert utils.coherence(T, 0, X, n_words=1, backend="host") == 0.0

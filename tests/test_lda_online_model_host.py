"""CPU-only: the float64 model of online variational Bayes LDA (tests/lda_online_model.py) on the planted corpus of
tests/online_model.py (6000 x 600, k = 10, alpha = 0.1, eta = 0.01, 10 % of every document's tokens held out) decides the
defaults of enstop_amd/lda_online.py: with n_batches = 64, doc_iter = 3, kappa = 0.7 and tau0 = 10, EPOCHS is the smallest
epoch count (5 at the most) after which the held-out perplexity is at least 2 % below batch LDA's after 20 iterations from the
same start, and doc_iter = 1 -- the batch fit's default -- does not get there in 5 epochs.  The device is held to this model
in tests/test_lda_online.py."""
import inspect

import numpy as np

import lda_online_model as M


def test_epochs_is_the_smallest_count_that_beats_twenty_batch_iterations():
    batch = M.batch_perplexity()
    online = M.model()["online_perplexity"]
    print("\nheld-out perplexity: 20 batch iterations %.1f, 40: %.1f; online after 1 .. 5 epochs: %s"
          % (batch, M.batch_perplexity(40), ", ".join("%.1f" % p for p in online)))
    assert len(online) == M.FIT["max_epochs"] == 5
    enough = [e + 1 for e, p in enumerate(online) if p <= (1.0 - M.ROOM) * batch]
    assert enough and enough[0] == M.EPOCHS, (enough, online, batch)
    # more batch iterations do not close the gap: the batch fit has converged where it is
    assert online[M.EPOCHS - 1] <= (1.0 - M.ROOM) * M.batch_perplexity(40)


def test_one_round_per_step_does_not_get_there():
    batch = M.batch_perplexity()
    online = M.model(doc_iter=1)["online_perplexity"]
    print("\ndoc_iter = 1, online after 1 .. 5 epochs: %s (batch %.1f)" % (", ".join("%.1f" % p for p in online), batch))
    assert all(p > (1.0 - M.ROOM) * batch for p in online), (online, batch)


def test_the_model_runs_the_schedule_and_the_bound_of_the_package():
    m = M.model()
    steps = M.FIT["n_batches"] * M.FIT["max_epochs"]
    assert len(m["rho"]) == steps and len(m["L"]) == M.FIT["max_epochs"]
    from enstop_amd.online import OnlineSchedule
    s = OnlineSchedule(M.FIT["n_batches"], M.FIT["max_epochs"], M.FIT["kappa"], M.FIT["tau0"], None, 0.0)
    assert [s.rho_at(t) for t in range(steps)] == m["rho"]
    assert (np.diff(m["L"]) > 0).all()               # the progressive bound rises from epoch to epoch
    assert sorted(m["perm"]) == list(range(M.the_split()[0].shape[0]))


def test_the_defaults_of_the_package_are_the_settings_of_the_model():
    from enstop_amd.lda_online import OnlineLDA, lda_fit_online
    defaults = {name: p.default for name, p in inspect.signature(lda_fit_online).parameters.items()}
    for name in ("n_batches", "doc_iter", "kappa", "tau0"):
        assert defaults[name] == M.FIT[name], name
        assert OnlineLDA().get_params()[name] == M.FIT[name], name
    assert defaults["n_epochs"] == M.FIT["max_epochs"] and defaults["rho"] is None

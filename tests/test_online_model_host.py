"""CPU: the float64 restatement of stepwise EM (tests/online_model.py) on the planted 6000 x 600 corpus, before anything runs
on a device.  It shows that the corpus and the settings of the end-to-end test (tests/test_online_em.py) are ones on which the
algorithm itself does what the device is then asked to do: after EPOCHS epochs of 64 blocks (kappa = 0.7, tau0 = 10,
inner_iter = 3) the held-out perplexity, taken under the final-fold P(z|d), is at least 2 % below batch EM's after 20
iterations from the same factors -- and EPOCHS is the smallest such count.

Figures of the model (split_documents(X, 0.9, RandomState(0)), then plsa_init from the same stream):
    batch EM, 10 / 20 / 40 iterations:   385.3 / 300.3 / 323.9
    stepwise, after 1 .. 5 epochs:       311.5, 274.2, 271.2, 272.9, 275.6
"""
import numpy as np

import online_model as om


def test_the_corpus_and_the_split_are_the_stated_ones():
    X = om.planted_corpus()
    assert X.shape == (6000, 600) and (np.asarray(X.sum(1)).ravel() == 40).all()
    observed, held, scored, U0, V0 = om.the_split()
    assert (observed + held != X).nnz == 0 and 0.09 < held.sum() / X.sum() < 0.11
    assert U0.shape == (6000, 10) and V0.shape == (10, 600) and U0.dtype == np.float32
    assert scored.sum() >= 5500
    seen = np.asarray(observed.sum(0)).ravel() > 0
    assert held[:, ~seen].sum() == 0                     # no held-out token of a word the observed part never shows


def test_the_block_cut_is_row_ranges_by_nnz():
    from enstop_amd.sharded import row_ranges_by_nnz
    observed = om.the_split()[0]
    for parts in (1, 3, 64):
        assert om.row_ranges(observed.indptr, parts) == row_ranges_by_nnz(observed.indptr, parts)


def test_the_step_sizes_and_the_progressive_likelihood():
    m = om.model()
    t = np.arange(64 * om.FIT["max_epochs"])
    np.testing.assert_allclose(m["rho"], (10.0 + t) ** -0.7, rtol=1e-15)
    L = np.array(m["L"])
    assert len(L) == 5 and (np.diff(L) > 0).all()        # every epoch's progressive likelihood is above the one before


def test_stepwise_em_beats_twenty_batch_iterations_after_the_stated_epochs_with_room():
    m = om.model()
    curve, batch = m["online_perplexity"], m["batch_perplexity"]
    print("\nbatch EM after %d iterations: %.2f; stepwise after 1 .. 5 epochs: %s"
          % (om.FIT["batch_iterations"], batch, ", ".join("%.2f" % p for p in curve)))
    enough = [E for E in range(1, om.FIT["max_epochs"] + 1) if curve[E - 1] <= (1.0 - om.ROOM) * batch]
    assert enough and enough[0] == om.EPOCHS, (enough, curve, batch)
    assert curve[om.EPOCHS - 1] <= (1.0 - om.ROOM) * batch


def test_one_block_one_epoch_at_rho_one_is_one_batch_iteration():
    """the restatement against itself: a single block, inner_iter = 0 and a step size of 1 (tau0 = 1, t = 0) make the
    statistic the block's sums, so the topics are batch EM's after one iteration"""
    observed, _, _, U0, V0 = om.the_split()
    X = observed[:500]
    factors, _, rhos = om.stepwise(X, U0[:500], V0, 1, 1, 0, 0.7, 1.0)
    assert rhos == [1.0]
    _, Vb = om.batch_em(X, U0[:500], V0, 1)
    np.testing.assert_allclose(factors[0][1], Vb, rtol=1e-12, atol=0)

"""A context gives its device memory back when it is destroyed (vbfm_destroy: store_release,
csrc/vbfm_store.hip, and the other groups' releases). The deferred split's payload -- 8 B per
train entry here, every x being 1 -- is a build product of the store that only the store's own
release knows; a destroy that freed a list of its own leaked it on every create / destroy cycle.

One cycle: create, train and test set, init caches, one iteration, close. After a warm-up cycle
(code objects, the runtime's first-use pools) four more cycles may not lower the device's free
memory by as much as one payload; four leaked payloads are at least four times that.
VBFM_FORCE_SPLIT=1 builds the split forms on one rank, VBFM_PLACE=0 keeps the placement search
(and its transient buffers) out.

The online learner owns its buffers through its state (OvState, csrc/vbfm_online.h), so an init that
fails half way, a second init on a live context and close() all release through one destructor:
test_online_init_failure_and_reinit."""
import numpy as np
import pytest
import torch

import online_cases as ocs
import vbfm

pytestmark = pytest.mark.gpu

N_ROWS, FIELDS, IDS, K = 200_000, 6, 400, 2
PAYLOAD = N_ROWS * FIELDS * 8   # nnz x 8 B


def _cycle(learner, layout):
    D = FIELDS * IDS + 1
    if learner == "vb":
        g = vbfm.FMLearnVB(1, 1, K, D, layout=layout)
    else:
        g = vbfm.FMLearnMCMC(1, 1, K, D, method="mcmc", layout=layout)
    try:
        g.init_device(7)
        g.synth(0, N_ROWS, FIELDS, IDS, 41)
        g.synth(1, 1000, FIELDS, IDS, 42)
        g.init_caches()
        g.iterate()
        assert g.layout() == layout
    finally:
        g.close()


@pytest.mark.parametrize("layout", ["level", "entry"])
@pytest.mark.parametrize("learner", ["vb", "mcmc"])
def test_destroy_returns_device_memory(monkeypatch, learner, layout):
    for kk in ("VBFM_LAYOUT", "VBFM_DEFER", "VBFM_ESTORE", "VBFM_FAULT"):
        monkeypatch.delenv(kk, raising=False)
    monkeypatch.setenv("VBFM_FORCE_SPLIT", "1")
    monkeypatch.setenv("VBFM_PLACE", "0")
    if layout == "entry":
        monkeypatch.setenv("VBFM_DEFER", "1")   # the entry store's split is two-pass unless asked
    _cycle(learner, layout)
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(4):
        _cycle(learner, layout)
    drop = free0 - torch.cuda.mem_get_info()[0]
    print("free memory drop over 4 cycles: %d B = %.2f payloads" % (drop, drop / PAYLOAD))
    assert drop < PAYLOAD


def _online_learner():
    tr, te, nf, nft, D = ocs.data("g4", 1)
    train, test = vbfm.DataSubset.from_csr(*tr, nf), vbfm.DataSubset.from_csr(*te, nft)
    g = vbfm.FMLearnVBOnline(1, 1, 3, D, min_target=train.min_target, max_target=train.max_target)
    g.set_data(train, test)
    return g


def _online_epochs(g, nb):
    """Three epochs' statistics and the state they leave, for exact comparison."""
    stats = []
    for _ in range(3):
        st = g.epoch()
        assert st.num_batch == nb and st.n_lord_batches == nb
        stats.append((st.rmse, st.mae, st.free_energy_first, st.free_energy_last, st.alpha, st.sigma_0,
                      st.mu_0_dash, st.sigma_0_dash, st.n_pad_batches))
    return stats, g.get_params(), g.online_state(), np.array(g.predict())


def _assert_same_run(got, want, what):
    assert got[0] == want[0], what
    for part in (1, 2):
        assert set(got[part]) == set(want[part])
        for key, v in want[part].items():
            np.testing.assert_array_equal(np.asarray(got[part][key]), np.asarray(v), err_msg="%s %s" % (what, key))
    np.testing.assert_array_equal(got[3], want[3], err_msg=what)


def test_online_init_failure_and_reinit(monkeypatch):
    """VBFM_FAULT=online_init makes vbfm_online_init throw, as a failed HIP call would, once the learner
    state and the regroup buffers are allocated. The init fails with a message; the same context then
    initialises and runs three epochs bit for bit as a fresh one does; a second init with two batches
    on the live learner equals a fresh two-batch learner; closing twice is harmless."""
    for var in ocs.ONLINE_ENV + ("VBFM_FAULT",):
        monkeypatch.delenv(var, raising=False)
    fresh = {}
    for nb in (1, 2):
        g = _online_learner()
        g.init(ocs.SEED, ocs.INIT_STDEV, nb)
        fresh[nb] = _online_epochs(g, nb)
        g.close()
    g = _online_learner()
    try:
        monkeypatch.setenv("VBFM_FAULT", "online_init")
        with pytest.raises(vbfm.VbfmError) as err:
            g.init(ocs.SEED, ocs.INIT_STDEV, 1)
        assert "online_init" in str(err.value), str(err.value)
        with pytest.raises(vbfm.VbfmError, match="not an online VB context"):
            g.epoch()
        monkeypatch.delenv("VBFM_FAULT")
        g.init(ocs.SEED, ocs.INIT_STDEV, 1)
        _assert_same_run(_online_epochs(g, 1), fresh[1], "after a failed init")
        g.init(ocs.SEED, ocs.INIT_STDEV, 2)
        _assert_same_run(_online_epochs(g, 2), fresh[2], "second init on a live learner")
    finally:
        g.close()
        g.close()

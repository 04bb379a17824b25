"""A context gives its device memory back when it is destroyed: every device pointer it holds is
an owner (DevBuf, csrc/vbfm_ctx.h) or a view of one, and vbfm_destroy is a delete. The deferred
split's payload -- 8 B per train entry here, every x being 1 -- is a build product of the store;
a destroy that freed a list of its own once leaked it on every create / destroy cycle.

One cycle: create, train and test set, init caches, one iteration, close. After a warm-up cycle
(code objects, the runtime's first-use pools) four more cycles may not lower the device's free
memory by as much as one payload; four leaked payloads are at least four times that.
VBFM_FORCE_SPLIT=1 builds the split forms on one rank, VBFM_PLACE=0 keeps the placement search
(and its transient buffers) out.

The online learner owns its buffers through its state (OvState, csrc/vbfm_online.h), so an init that
fails half way, a second init on a live context and close() all release through one destructor:
test_online_init_failure_and_reinit.

The same accounting for what is released while a context lives: a replay init that fails with its
buffers allocated, data sets replaced on a live context, and the handles (models, candidate sets,
chains of draws)."""
import numpy as np
import pytest
import torch

import online_cases as ocs
import recommend_cases as rc
import vbfm

pytestmark = pytest.mark.gpu

N_ROWS, FIELDS, IDS, K = 200_000, 6, 400, 2
PAYLOAD = N_ROWS * FIELDS * 8   # nnz x 8 B


D_ALL = FIELDS * IDS + 1


def _free():
    return torch.cuda.mem_get_info()[0]


def _cycle(learner, layout):
    if learner == "online":
        g = vbfm.FMLearnVBOnline(1, 1, K, D_ALL)
    elif learner == "mcmc":
        g = vbfm.FMLearnMCMC(1, 1, K, D_ALL, method="mcmc", layout=layout)
    else:
        g = vbfm.FMLearnVB(1, 1, K, D_ALL, layout=layout)
    try:
        if learner == "vb_fshards":   # owns the shards' base / buf / rows0
            g.set_shard_mode("features", 2)
        if learner != "online":
            g.init_device(7)
        g.synth(0, N_ROWS, FIELDS, IDS, 41)
        g.synth(1, 1000, FIELDS, IDS, 42)
        if learner == "online":
            g.init(7, 0.1, 2)
            assert g.epoch().num_batch == 2
        else:
            g.init_caches()
            g.iterate()
        assert g.layout() == layout
    finally:
        g.close()


@pytest.mark.parametrize("learner,layout", [("vb", "level"), ("mcmc", "level"), ("vb", "entry"), ("mcmc", "entry"),
                                            ("vb_fshards", "column"), ("online", "column")])
def test_destroy_returns_device_memory(monkeypatch, learner, layout):
    for kk in ("VBFM_LAYOUT", "VBFM_DEFER", "VBFM_ESTORE", "VBFM_FAULT", "VBFM_FORCE_SPLIT"):
        monkeypatch.delenv(kk, raising=False)
    if layout != "column":
        monkeypatch.setenv("VBFM_FORCE_SPLIT", "1")
    monkeypatch.setenv("VBFM_PLACE", "0")
    if layout == "entry":
        monkeypatch.setenv("VBFM_DEFER", "1")   # the entry store's split is two-pass unless asked
    _cycle(learner, layout)
    free0 = _free()
    for _ in range(4):
        _cycle(learner, layout)
    drop = free0 - _free()
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


def test_failed_replay_init_returns_its_memory(monkeypatch):
    """VBFM_FAULT=replay makes the first attempt of vbfm_init_params_replay throw once the attempt's
    buffers, the stream-end word and the two output buffers are allocated. k = 8, D = 200,001, no data
    set: the init draws nnorm = 2 (k D + D) normals, and the attempt's uniform array alone is
    U = 4 B x 2.8 x nnorm, about 40 MB. After one failing call as warm-up, four more may not lower
    the free memory by U (buffers freed by hand at the bottom of the loop leaked more than 2 U per
    call). The same context then initialises bit for bit as a fresh one."""
    monkeypatch.delenv("VBFM_FAULT", raising=False)
    k, D, seed = 8, 200_001, 11
    U = int(4 * 2.8 * 2 * (k * D + D))

    def drawn(g):
        g.init_replay(seed, 0.1, keep_model_draws=True)
        return dict(g.get_params(), fm_v=g.fm_v, fm_w=g.fm_w)

    g = vbfm.FMLearnVB(1, 1, k, D)
    try:
        want = drawn(g)
    finally:
        g.close()
    g = vbfm.FMLearnVB(1, 1, k, D)
    try:
        monkeypatch.setenv("VBFM_FAULT", "replay")

        def failing_call():
            with pytest.raises(vbfm.VbfmError, match="VBFM_FAULT=replay"):
                g.init_replay(seed, 0.1, keep_model_draws=True)

        failing_call()
        free0 = _free()
        for _ in range(4):
            failing_call()
        drop = free0 - _free()
        print("free memory drop over 4 failed replay inits: %d B = %.2f U" % (drop, drop / U))
        assert drop < U
        monkeypatch.delenv("VBFM_FAULT")
        got = drawn(g)
        assert set(got) == set(want)
        for key, v in want.items():
            np.testing.assert_array_equal(np.asarray(got[key]), np.asarray(v), err_msg=key)
    finally:
        g.close()


def test_replacing_data_returns_the_old_set(monkeypatch):
    """One VB context on the level layout, six rounds of: the same parameters, a train and a test set
    generated anew, init caches, one iteration. Each round replaces both data sets, the records, the
    schedule's tables, the store and the test buffers of the round before on a live context. After two
    rounds, four more may not lower the free memory by one payload, and every round's RMSE is the
    first round's (the same data, the same seed)."""
    for kk in ("VBFM_LAYOUT", "VBFM_DEFER", "VBFM_ESTORE", "VBFM_FAULT", "VBFM_FORCE_SPLIT"):
        monkeypatch.delenv(kk, raising=False)
    monkeypatch.setenv("VBFM_PLACE", "0")
    g = vbfm.FMLearnVB(1, 1, K, D_ALL, layout="level")
    try:
        def one_round():
            g.init_device(7)
            g.synth(0, N_ROWS, FIELDS, IDS, 41)
            g.synth(1, 1000, FIELDS, IDS, 42)
            g.init_caches()
            st = g.iterate()
            assert g.layout() == "level"
            return st.rmse

        rmse = [one_round(), one_round()]
        free0 = _free()
        rmse += [one_round() for _ in range(4)]
        drop = free0 - _free()
        print("free memory drop over 4 replacements: %d B = %.2f payloads" % (drop, drop / PAYLOAD))
        assert drop < PAYLOAD
        assert rmse == [rmse[0]] * 6, rmse
    finally:
        g.close()


def test_handles_return_device_memory(monkeypatch):
    """Models, candidate sets and chains of draws own their device memory the same way. One cycle on a
    trained VB learner (k = 8) and an MCMC learner: a model from the learner, a candidate set of
    M = 100,000 rows with the variance planes (3 M (k + 1) 8 B = C, about 21 MB), a ranking for 64
    contexts, the scores of 10,000 rows, a chain of capacity 4 with two draws made into a model; all
    closed. After a warm-up cycle four more may not lower the free memory by C, and the last cycle's
    rankings and scores are the first's bit for bit."""
    for kk in ("VBFM_LAYOUT", "VBFM_DEFER", "VBFM_ESTORE", "VBFM_FAULT", "VBFM_FORCE_SPLIT"):
        monkeypatch.delenv(kk, raising=False)
    k, M = 8, 100_000
    C = 3 * M * (k + 1) * 8
    ctx, cand, rows = rc.contexts(64), rc.candidates(M, D=D_ALL), rc.contexts(10_000, seed=4)

    def trained(cls, **kw):
        g = cls(1, 1, k, D_ALL, **kw)
        g.init_device(7)
        g.synth(0, 20_000, FIELDS, IDS, 41)
        g.synth(1, 1000, FIELDS, IDS, 42)
        g.init_caches()
        g.iterate()
        return g

    vb, mc = trained(vbfm.FMLearnVB), trained(vbfm.FMLearnMCMC, method="mcmc")
    try:
        def cycle():
            m = vbfm.Model.from_learner(vb)
            cs = m.candidates(cand, variance=True)
            ranked = m.recommend(ctx, cs, 10)
            scores = m.score(rows)
            ch = mc.chain(4)
            ch.add()
            ch.add()
            cm = ch.model()
            chain_scores = cm.score(rows)
            for h in (cm, ch, cs, m):
                h.close()
            return ranked + (scores, chain_scores)

        first = cycle()
        free0 = _free()
        for _ in range(4):
            last = cycle()
        drop = free0 - _free()
        print("free memory drop over 4 handle cycles: %d B = %.2f C" % (drop, drop / C))
        assert drop < C
        assert rc.same(first, last)
    finally:
        vb.close()
        mc.close()

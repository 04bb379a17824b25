"""Chains of draws on the GPU (include/vbfm.h "chains of draws"): the collector, the model of kind
mcmc_chain and its scores -- the mean over the draws of the per-draw predictions and their spread.

The definition is restated here in plain float64 (restate): mean and var follow from the per-draw
scores that one-draw MCMC_DRAW models give through the existing scorer, so every comparison with it
is byte for byte. Nothing is trained where the draws can come from numpy.
"""
import ctypes
import os
import queue
import re
import subprocess

import numpy as np
import pytest

import class_ref as cr
import vbfm
from conftest import GOLDEN, ROOT, load_case

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "scalable-variational-bayesian-factorization-machine_amd", "bin", "libFM")
PRINT_REL = 6e-6          # tests/test_class_gpu.py: the reference prints 6 significant digits
D = 50
MN, MX = -1.0, 2.0        # the regression models' target range: narrow enough to clip some scores


def restate(p, lo=None, hi=None):
    """mean and var of include/vbfm.h from the per-draw p_s [S][n], operation by operation."""
    S = len(p)
    total = np.zeros_like(p[0])
    for s in range(S):
        total = total + p[s]
    mean = total / S
    if lo is not None:
        mean = np.maximum(lo, np.minimum(hi, mean))
    m, M2 = np.zeros_like(p[0]), np.zeros_like(p[0])
    for s in range(S):
        d = p[s] - m
        m = m + d / (s + 1)
        M2 = M2 + d * (p[s] - m)
    return mean, M2 / S


def clip_r(y):
    return np.maximum(MN, np.minimum(MX, y))


# ---- rows: every length that crosses a boundary of the kernels' entry loops -----------------------
LENGTHS = [0, 1, 2, 7, 8, 9, 63, 64, 65, 130]


EXTRA = [3, 5, 4, 11, 6, 2, 10, 1, 0, 9, 8, 7, 3, 5, 12, 4, 6, 2, 1, 11, 10, 3, 7, 5, 4, 6, 2]   # 37 rows in all


def make_rows():
    rng = np.random.default_rng(3)
    lens = LENGTHS + EXTRA
    assert len(lens) == 37
    feat, val = [], []
    for i, n in enumerate(lens):
        f = np.sort(rng.integers(0, D, size=n)).astype(np.uint32)
        if i == 12:
            f = np.unique(f)[::-1].copy()           # a row given in descending id
            lens[i] = n = len(f)
        if i == 13:
            f[1] = f[0]                             # a row with a repeated id
        feat.append(f)
        val.append(rng.uniform(-1.5, 1.5, size=n).astype(np.float32))
    rp = np.zeros(len(lens) + 1, dtype=np.uint64)
    np.cumsum(lens, out=rp[1:])
    return rp, np.concatenate(feat), np.concatenate(val)


ROWS = make_rows()


def rows():
    return ROWS


def make_draws(k, S, seed):
    rng = np.random.default_rng(seed)
    return [dict(w=rng.normal(0, 0.3, D), v=rng.normal(0, 0.3, k * D), w0=float(rng.normal(0, 0.5)),
                 alpha=float(rng.uniform(0.5, 3.0))) for _ in range(S)]


def info_of(kind, k, k0, k1, task):
    mn, mx = (-1.0, 1.0) if task == "c" else (MN, MX)
    return dict(kind=kind, k0=k0, k1=k1, num_factor=k, num_attribute=D, min_target=mn, max_target=mx, iter=7)


def load_models(tmp_path, k, S, k0, k1, task, seed):
    """One chain model and the S one-draw models of the same numbers."""
    draws = make_draws(k, S, seed)
    cpath = str(tmp_path / ("chain_%s" % task))
    vbfm.Model.write_chain(cpath, info_of(4, k, k0, k1, task), draws, task=task)
    chain = vbfm.Model.load(cpath)
    ones = []
    for s, d in enumerate(draws):
        p = str(tmp_path / ("draw_%s_%d" % (task, s)))
        info = info_of(3, k, k0, k1, task)
        info.update(w0_or_mu0=d["w0"], alpha=d["alpha"])
        vbfm.Model.write_params(p, info, d, task=task)
        ones.append(vbfm.Model.load(p))
    return chain, ones, draws


def expected(ones, data, order, clip, task, unknown_ids="refuse"):
    """The restatement over the one-draw models' scores. Task c with clip: p_s is the one-draw model's
    own clip = 1 score (the library's link on the device), not a second Phi."""
    if task == "c" and clip:
        p = [m.score(data, order=order, clip=True, unknown_ids=unknown_ids) for m in ones]
        return restate(p, 0.0, 1.0)
    y = [m.score(data, order=order, clip=False, unknown_ids=unknown_ids) for m in ones]
    if clip:
        return restate([clip_r(v) for v in y], MN, MX)
    return restate(y)


# every k with an S that is no multiple of the draws one pass of its instantiation takes (8, 4, 4, 4,
# 2 for k <= 8, 16, 32, 64, 256) and with one above it; k0 / k1 alternate
SHAPES = [(0, 3, 1, 1), (0, 9, 0, 1), (1, 1, 1, 1), (1, 9, 1, 0), (3, 2, 1, 1), (3, 17, 0, 0), (8, 3, 1, 1), (8, 8, 1, 1),
          (8, 9, 0, 1), (8, 17, 1, 1), (9, 3, 1, 1), (9, 9, 1, 0), (16, 2, 1, 1), (16, 17, 1, 1), (17, 3, 0, 1),
          (17, 9, 1, 1), (33, 1, 1, 1), (33, 9, 1, 1), (64, 3, 1, 0), (64, 17, 1, 1), (65, 1, 1, 1), (65, 3, 1, 1),
          (65, 9, 0, 1), (130, 3, 1, 1), (130, 17, 1, 1)]


@pytest.mark.parametrize("k,S,k0,k1", SHAPES)
def test_chain_scores_are_the_restatement_of_the_one_draw_scores(k, S, k0, k1, tmp_path, monkeypatch):
    """For every (order, clip, task): chain.score(rows, variance=True) equals, byte for byte, the
    definition applied to the scores of S one-draw MCMC_DRAW models holding the same numbers. Order
    group in both of its geometries (VBFM_CHAIN_LOOP: the draws across the wave, the per-draw loop)."""
    data = rows()
    for task in ("r", "c"):
        chain, ones, draws = load_models(tmp_path, k, S, k0, k1, task, seed=100 + k + S)
        assert chain.num_draws == S and chain.info["kind"] == 4 and chain.task == task
        assert chain.info["has_variance"] == 0
        w0, alpha = chain.draw_scalars()
        assert w0.tolist() == [d["w0"] for d in draws] and alpha.tolist() == [d["alpha"] for d in draws]
        assert chain.info["w0_or_mu0"] == draws[-1]["w0"] and chain.info["alpha"] == draws[-1]["alpha"]
        for order, loop in (("exact", None), ("group", "0"), ("group", "1"), ("auto", None)):
            if loop is None:
                monkeypatch.delenv("VBFM_CHAIN_LOOP", raising=False)
            else:
                monkeypatch.setenv("VBFM_CHAIN_LOOP", loop)
            for clip in (False, True):
                mean, var = chain.score(data, variance=True, order=order, clip=clip)
                em, ev = expected(ones, data, "exact" if order == "auto" else order, clip, task)
                worst = float(np.max(np.abs(mean - em))) if len(em) else 0.0
                print(task, order, loop, clip, "max |mean - restated|", worst, "max var", float(var.max()))
                assert mean.tobytes() == em.tobytes(), (task, order, loop, clip, worst)
                assert var.tobytes() == ev.tobytes(), (task, order, loop, clip)
                assert np.all(var >= 0)
                if S == 1:
                    assert not var.any()
                assert chain.score(data, order=order, clip=clip).tobytes() == mean.tobytes()   # without var
        if S > 1 and k > 0:
            assert chain.score(data, variance=True, clip=False)[1].max() > 0
        for m in ones + [chain]:
            m.close()


@pytest.mark.parametrize("k,S", [(8, 9), (65, 3)])
def test_chunks_and_geometry_give_identical_bytes(k, S, tmp_path, monkeypatch):
    data = rows()
    chain, ones, _ = load_models(tmp_path, k, S, 1, 1, "r", seed=5)
    for order in ("group", "exact"):
        base = chain.score(data, variance=True, order=order)
        assert chain.last_stats["n_chunks"] == 1
        for chunk in (1, 300, 4096):
            got = chain.score(data, variance=True, order=order, chunk_bytes=chunk)
            if chunk == 1:
                assert chain.last_stats["n_chunks"] == 37   # one row per chunk
            assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes(), (order, chunk)
    base = chain.score(data, variance=True, order="group")
    for loop in ("0", "1"):   # the draws across the wave / the per-draw loop, whichever the library picks
        monkeypatch.setenv("VBFM_CHAIN_LOOP", loop)
        got = chain.score(data, variance=True, order="group")
        assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes(), loop
    monkeypatch.delenv("VBFM_CHAIN_LOOP")
    for g in ("16", "32", "64"):
        monkeypatch.setenv("VBFM_SCORE_G", g)
        got = chain.score(data, variance=True, order="group")
        assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes(), g
    for m in ones + [chain]:
        m.close()


@pytest.mark.parametrize("loop", ["0", "1"])
def test_unknown_ids(tmp_path, monkeypatch, loop):
    monkeypatch.setenv("VBFM_CHAIN_LOOP", loop)
    rp, feat, val = rows()
    feat = feat.copy()
    rp_i = rp.astype(np.int64)
    # three unknown entries: two in row 9 (130 entries), one in row 5
    feat[rp_i[9] + 3] = D + 4
    feat[rp_i[9] + 77] = D + 2
    feat[rp_i[5] + 1] = D + 9
    data = (rp, feat, val)
    for k, S in ((8, 9), (65, 3)):
        chain, ones, _ = load_models(tmp_path, k, S, 1, 1, "r", seed=9)
        for order in ("group", "exact"):
            with pytest.raises(vbfm.VbfmError, match=r"row 5 holds feature id %d" % (D + 9)):
                chain.score(data, order=order)
            mean, var = chain.score(data, variance=True, order=order, unknown_ids="skip")
            assert chain.last_stats["skipped_entries"] == 3   # each entry once, not once per draw
            em, ev = expected(ones, data, order, True, "r", unknown_ids="skip")
            assert mean.tobytes() == em.tobytes() and var.tobytes() == ev.tobytes(), (k, S, order)
        for m in ones + [chain]:
            m.close()


# ---- the chain average is training's ---------------------------------------------------------------
def tiny_learner(case="tiny/mcmc"):
    t, _ = load_case(case)
    m = t["meta"]
    d = os.path.join(GOLDEN, "tiny")
    train, test = vbfm.DataSubset.load(os.path.join(d, "train.libfm")), vbfm.DataSubset.load(os.path.join(d, "test.libfm"))
    k0, k1, k = [int(x) for x in m["dim"].split(",")]
    fml = vbfm.FMLearnMCMC(k0, k1, k, vbfm.num_all_attribute(train, test), min_target=train.min_target,
                           max_target=train.max_target, method="mcmc")
    fml.init(m["seed"], m["init_stdev"], regular=m.get("regular", ()))
    fml.set_data(train, test)
    fml.init_caches()
    return fml, train, test, m


def test_the_chain_average_is_what_training_reports(tmp_path):
    """tiny/mcmc on the reference stream with every draw kept: the chain model's scores of the test
    rows are fml.predict() byte for byte, from the collector and from its file; rmse_all follows."""
    fml, train, test, m = tiny_learner()
    ch = fml.chain(m["iter"])
    assert len(ch) == 0
    with pytest.raises(vbfm.VbfmError, match="no draw"):
        ch.model()
    for i in range(m["iter"]):
        st = fml.iterate()
        ch.add()
        assert len(ch) == i + 1
    pred = fml.predict()
    model = ch.model()
    assert model.num_draws == m["iter"] and model.info["kind"] == 4
    got = model.score(test)
    print("max |score - predict|", float(np.max(np.abs(got - pred))))
    assert got.tobytes() == pred.tobytes()
    assert model.score_device(fml, 1).tobytes() == pred.tobytes()
    mean, var = model.score(test, variance=True)
    assert mean.tobytes() == pred.tobytes() and np.all(var >= 0) and var.max() > 0
    dm, dv = model.score_device(fml, 1, variance=True)
    assert dm.tobytes() == mean.tobytes() and dv.tobytes() == var.tobytes()
    path = str(tmp_path / "chain.vbfm")
    ch.save(path)
    assert vbfm.Model.file_draws(path) == m["iter"] and vbfm.Model.file_info(path)["iter"] == m["iter"]
    loaded = vbfm.Model.load(path)
    assert loaded.score(test).tobytes() == pred.tobytes()
    assert loaded.draw_scalars()[1][-1] == st.alpha and loaded.info["alpha"] == st.alpha
    # the last draw of the file is the learner's parameters as they are
    p = fml.get_params()
    last = vbfm.Model.read_draw(path, m["iter"] - 1)
    assert last["w"].tobytes() == p["w"].tobytes() and last["v"].tobytes() == p["v"].tobytes() and last["w0"] == p["w0"]
    rmse = float(np.sqrt(np.mean((got - test.target.astype(np.float64)) ** 2)))
    print("rmse_all", st.rmse_all, "from the chain's scores", rmse)
    assert abs(rmse - st.rmse_all) <= 1e-12 * st.rmse_all
    # beyond the capacity, and the other refusals of the collector
    with pytest.raises(vbfm.VbfmError, match="full"):
        ch.add()
    for x in (model, loaded, ch, fml):
        x.close()


def test_burn_in_and_thinning(tmp_path):
    """add() only at i >= 2 and (i - 2) % 3 == 0: the restatement over exactly those draws, snapshot
    with Model.from_learner at the same iterations. The collector is left partly filled (2 of 4):
    its model and its file hold the draws at their own stride."""
    fml, train, test, m = tiny_learner()
    ch = fml.chain(4)
    snaps = []
    for i in range(m["iter"]):
        fml.iterate()
        if i >= 2 and (i - 2) % 3 == 0:
            ch.add()
            snaps.append(vbfm.Model.from_learner(fml))
    assert len(ch) == len(snaps) == 2
    model = ch.model()
    mean, var = model.score(test, variance=True)
    y = [s.score(test, clip=False) for s in snaps]
    lo, hi = float(train.min_target), float(train.max_target)
    em, ev = restate([np.maximum(lo, np.minimum(hi, v)) for v in y], lo, hi)
    assert mean.tobytes() == em.tobytes() and var.tobytes() == ev.tobytes()
    path = str(tmp_path / "partly.vbfm")
    ch.save(path)
    assert vbfm.Model.file_draws(path) == 2
    p = fml.get_params()   # the second kept draw is iteration 5's, the learner's parameters as they are
    last = vbfm.Model.read_draw(path, 1)
    assert last["w"].tobytes() == p["w"].tobytes() and last["v"].tobytes() == p["v"].tobytes()
    loaded = vbfm.Model.load(path)
    lm, lv = loaded.score(test, variance=True)
    assert lm.tobytes() == em.tobytes() and lv.tobytes() == ev.tobytes()
    with pytest.raises(vbfm.VbfmError, match="draw 2 of a model of 2"):
        loaded._mcheck(vbfm.lib().vbfm_model_draw_scalars(loaded._m, 2, None, None))   # (the model's own error slot)
    for x in snaps + [model, loaded, ch, fml]:
        x.close()


@pytest.fixture(scope="module")
def cls_tiny(tmp_path_factory):
    t = cr.load_trace("cls_tiny/mcmc")
    return t, cr.case_files(tmp_path_factory.mktemp("cls_chain"), t["meta"]["data"], t["meta"]["threshold"])


def cls_learner(t, files, rng=vbfm.RNG_REFERENCE):
    m = t["meta"]
    train, test = vbfm.DataSubset.load(files["train"]), vbfm.DataSubset.load(files["test"])
    k0, k1, k = m["dim"]
    fml = vbfm.FMLearnMCMC(k0, k1, k, vbfm.num_all_attribute(train, test), min_target=train.min_target,
                           max_target=train.max_target, method="mcmc", task="c")
    fml.init(m["seed"], m["init_stdev"], regular=m["regular"], rng=rng)
    return fml, train, test


def test_classification_against_the_reference(cls_tiny):
    """cls_tiny/mcmc with every draw kept: clip = 1 scores are fml.predict() byte for byte and the
    reference CLI's recorded -out to its print precision; clip = 0 is the mean of the raw yhat_s."""
    t, files = cls_tiny
    fml, train, test = cls_learner(t, files)
    fml.set_data(train, test)
    fml.init_caches()
    ch = fml.chain(t["meta"]["iter"])
    snaps = []
    for _ in range(t["meta"]["iter"]):
        fml.iterate()
        ch.add()
        snaps.append(vbfm.Model.from_learner(fml))
    model = ch.model()
    assert model.task == "c"
    prob = model.score(test, clip=True)
    assert prob.tobytes() == fml.predict().tobytes()
    ref = np.asarray(t["pred"])
    err = float(np.max(np.abs(prob - ref) / np.abs(ref)))
    print("max relative difference to the reference's -out", err)
    assert err <= PRINT_REL
    raw, var = model.score(test, variance=True, clip=False)
    em, ev = restate([s.score(test, clip=False) for s in snaps])
    assert raw.tobytes() == em.tobytes() and var.tobytes() == ev.tobytes()
    assert not np.array_equal(raw, prob)
    for x in snaps + [model, ch, fml]:
        x.close()


def _cli(cwd, *args):
    return subprocess.run([CLI] + list(args), cwd=str(cwd), capture_output=True, text=True, timeout=300)


@pytest.mark.skipif(not os.path.exists(CLI), reason="bin/libFM not built")
def test_cli_chain(tmp_path):
    d = os.path.join(GOLDEN, "tiny")
    tr, te = os.path.join(d, "train.libfm"), os.path.join(d, "test.libfm")
    base = ["-task", "r", "-train", tr, "-test", te, "-dim", "1,1,3", "-iter", "6", "-seed", "5", "-vfile", "0"]
    r = _cli(tmp_path, *base, "-method", "mcmc", "-out", "pred.txt", "-save_model", "m", "-chain", "0,1")
    assert "ERROR" not in r.stderr, r.stderr
    assert vbfm.Model.file_draws(str(tmp_path / "m")) == 6 and vbfm.Model.file_info(str(tmp_path / "m"))["kind"] == 4
    s = _cli(tmp_path, "-load_model", "m", "-test", te, "-out", "scored.txt", "-out_var", "var.txt")
    assert "ERROR" not in s.stderr, s.stderr
    assert re.search(r"\b6 draws\b", s.stdout), s.stdout
    pred, scored = np.loadtxt(str(tmp_path / "pred.txt")), np.loadtxt(str(tmp_path / "scored.txt"))
    assert np.max(np.abs(scored - pred) / np.abs(pred)) <= 2 * PRINT_REL   # both print 6 digits
    var = np.loadtxt(str(tmp_path / "var.txt"))
    assert len(var) == len(pred) and np.all(var >= 0) and var.any()
    r = _cli(tmp_path, *base, "-method", "mcmc", "-save_model", "m2", "-chain", "2,3")
    assert "ERROR" not in r.stderr and vbfm.Model.file_draws(str(tmp_path / "m2")) == 2, r.stderr
    # without -chain the file is the one-draw model it always was
    r = _cli(tmp_path, *base, "-method", "mcmc", "-save_model", "m1")
    assert "ERROR" not in r.stderr and vbfm.Model.file_info(str(tmp_path / "m1"))["kind"] == 3, r.stderr
    r = _cli(tmp_path, *base, "-method", "mcmc", "-save_state", "st")
    assert "ERROR" not in r.stderr and os.path.exists(str(tmp_path / "st")), r.stderr
    refused = [(["-method", "als", "-save_model", "x", "-chain", "0,1"], "-method mcmc"),
               (["-method", "vb", "-save_model", "x", "-chain", "0,1"], "-method mcmc"),
               (["-method", "mcmc", "-save_model", "x", "-chain", "0,1", "-resume", "st"], "-resume"),
               (["-method", "mcmc", "-chain", "0,1"], "-save_model"),
               (["-method", "mcmc", "-save_model", "x", "-chain", "6,1"], "keeps no draw")]
    for extra, word in refused:
        r = _cli(tmp_path, *base, *extra)
        assert "ERROR" in r.stderr and word in r.stderr, (extra, r.stderr)
        assert not os.path.exists(str(tmp_path / "x")) and not os.path.exists(str(tmp_path / "x.tmp")), extra


def test_refusals_on_the_device(tmp_path):
    d = os.path.join(GOLDEN, "tiny")
    train, test = vbfm.DataSubset.load(os.path.join(d, "train.libfm")), vbfm.DataSubset.load(os.path.join(d, "test.libfm"))
    Dn = vbfm.num_all_attribute(train, test)
    als = vbfm.FMLearnMCMC(1, 1, 3, Dn, method="als")
    als.init(5, 0.1)
    with pytest.raises(vbfm.VbfmError, match="ALS is deterministic"):
        als.chain(4)
    vb = vbfm.FMLearnVB(1, 1, 3, Dn)
    vb.init(5, 0.1)
    h = ctypes.c_void_p()
    with pytest.raises(vbfm.VbfmError, match="sampling MCMC context"):   # (only FMLearnMCMC has chain())
        vbfm._check(vbfm.lib().vbfm_chain_create(ctypes.byref(h), vb._ctx, 4), vb._ctx)
    assert not h.value
    fml = vbfm.FMLearnMCMC(1, 1, 3, Dn, method="mcmc")
    fml.init(5, 0.1)
    other = vbfm.FMLearnMCMC(1, 1, 4, Dn, method="mcmc")
    other.init(5, 0.1)
    ch = fml.chain(1)
    with pytest.raises(vbfm.VbfmError, match="is not the chain's"):
        ch.add(other)
    with pytest.raises(vbfm.VbfmError, match="sampling MCMC context"):
        ch.add(als)
    ch.add()
    with pytest.raises(vbfm.VbfmError, match="full"):
        ch.add()
    assert len(ch) == 1
    # a capacity no device holds: refused from the sizes alone, both figures in the message
    need = (2 ** 32 - 1) * (Dn * 4 * 8 + 16)
    with pytest.raises(vbfm.VbfmError, match=r"need %d bytes of device memory, \d+ are free" % need):
        fml.chain(2 ** 32 - 1)
    model = ch.model()
    data = (np.array([0, 2], dtype=np.uint64), np.array([1, 3], dtype=np.uint32), np.array([1.0, 0.5], dtype=np.float32))
    with pytest.raises(vbfm.VbfmError, match="scored, not ranked"):
        model.candidates(data)
    one = vbfm.Model.from_learner(fml)
    cands = one.candidates(data)
    with pytest.raises(vbfm.VbfmError, match="scored, not ranked"):
        model.recommend(data, cands, 1)
    with pytest.raises(vbfm.VbfmError, match="no variances"):
        one.score(data, variance=True)
    assert one.num_draws == 1
    mean, var = model.score(data, variance=True)
    assert mean.tobytes() == one.score(data).tobytes() and not var.any()   # a chain of one draw is that draw
    for x in (cands, one, model, ch, other, fml, vb, als):
        x.close()


# ---- two ranks on one GPU through the host exchange -------------------------------------------------
def _shard(ds, lo, hi):
    rp = ds.row_ptr.astype(np.int64)
    sl = slice(int(rp[lo]), int(rp[hi]))
    return vbfm.DataSubset.from_csr((rp[lo:hi + 1] - rp[lo]).astype(np.uint64), ds.row_ent["id"][sl],
                                    ds.row_ent["value"][sl], ds.target[lo:hi], ds.num_feature)


def _chain_run(fml, train, test, iters, path):
    fml.set_data(train, test)
    fml.init_caches()
    ch = fml.chain(iters)
    for _ in range(iters):
        fml.iterate()
        ch.add()
    ch.save(path)
    ch.close()


def _chain_worker(rank, world, store_path, files, iters, out_dir, out_q):
    try:
        import torch
        import torch.distributed as dist
        store = dist.FileStore(store_path, world)
        dist.init_process_group("gloo", store=store, rank=rank, world_size=world)

        def allreduce(arr, op):
            tt = torch.from_numpy(arr.astype(np.float64) if arr.dtype == np.uint32 else arr.copy())
            if arr.dtype == np.uint8:
                tt = tt.to(torch.int32)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX if op == "max" else dist.ReduceOp.SUM)
            arr[:] = tt.numpy().astype(arr.dtype)

        train, test = vbfm.DataSubset.load(files["train"]), vbfm.DataSubset.load(files["test"])
        N, Nt = train.num_cases, test.num_cases
        Dn = vbfm.num_all_attribute(train, test)

        def learner():
            fml = vbfm.FMLearnMCMC(1, 1, 4, Dn, min_target=-1.0, max_target=1.0, method="mcmc", task="c")
            fml.init(42, 0.1, rng=vbfm.RNG_DEVICE)
            return fml
        fml = learner()
        fml.comm_init_host(world, rank, allreduce)
        _chain_run(fml, _shard(train, rank * N // world, (rank + 1) * N // world),
                   _shard(test, rank * Nt // world, (rank + 1) * Nt // world), iters,
                   os.path.join(out_dir, "sharded_rank%d" % rank))
        fml.close()
        if rank == 0:
            ref = learner()
            _chain_run(ref, train, test, iters, os.path.join(out_dir, "single"))
            ref.close()
            msg = {}
            for name in ("sharded_rank0", "single"):
                m = vbfm.Model.load(os.path.join(out_dir, name))
                msg[name] = m.score(test, variance=True, clip=False, order="exact") + (m.num_draws,)
                m.close()
            out_q.put(msg)
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as exc:   # reported to the parent instead of a silent hang
        import traceback
        out_q.put({"error": "rank %d: %r\n%s" % (rank, exc, traceback.format_exc())})


def test_two_ranks_collect_and_rank_0_writes(cls_tiny, tmp_path):
    import torch.multiprocessing as mp
    t, files = cls_tiny
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    out_dir = str(tmp_path)
    procs = [ctx.Process(target=_chain_worker, args=(r, 2, str(tmp_path / "rendezvous"), files, 3, out_dir, q))
             for r in range(2)]
    for p in procs:
        p.start()
    try:
        msg = q.get(timeout=300)
    except queue.Empty:
        msg = {"error": "no result within 300 s"}
    for p in procs:
        p.join(timeout=30)
        if p.is_alive():
            p.kill()
            p.join()
    assert "error" not in msg, msg["error"]
    assert os.path.exists(os.path.join(out_dir, "sharded_rank0")) and not os.path.exists(os.path.join(out_dir, "sharded_rank1"))
    assert not os.path.exists(os.path.join(out_dir, "sharded_rank1.tmp"))
    (sm, sv, sn), (rm, rv, rn) = msg["sharded_rank0"], msg["single"]
    assert sn == rn == 3
    err = float(np.max(np.abs(sm - rm)) / np.max(np.abs(rm)))
    print("mean: relative difference of the sharded chain", err)
    assert err <= 1e-9
    assert float(np.max(np.abs(sv - rv))) <= 1e-9 * float(np.max(rv))

"""Binary classification (-task c, probit link) of the MCMC / ALS learner on the GPU, against the
compiled reference's `-task c -method mcmc | als` runs (tests/golden/cls_*, written by
tests/golden/make_cls_golden.py from the unmodified reference binary).

The reference prints 6 significant digits, so a value is held to 6e-6 relative (+-5e-6 of print
rounding plus the suite's 1e-9 chain bound) and a correct count, round(printed * N) with
N <= 90,000, exactly. A sampled chain that takes one rand() too many or too few parts from the
reference's by O(1) within an iteration, so these bounds are decisive for the stream order.
"""
import math
import os
import queue
import subprocess
import sys

import numpy as np
import pytest

import class_ref as cr
import vbfm
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CLI = os.path.join(ROOT, "scalable-variational-bayesian-factorization-machine_amd", "bin", "libFM")
PRINT_REL = 6e-6
CASES = ["cls_tiny/mcmc", "cls_tiny/als_reg", "cls_sa/mcmc", "cls_sa/als_reg", "cls_tiny_dup/mcmc"]


@pytest.fixture(scope="session")
def cls_files(tmp_path_factory):
    """The fixtures' inputs with target >= threshold -> 1, else -1, written once."""
    d = tmp_path_factory.mktemp("cls")
    made = {}

    def get(trace):
        m = trace["meta"]
        if m["data"] not in made:
            made[m["data"]] = cr.case_files(d, m["data"], m["threshold"])
        return made[m["data"]]
    return get


_DATA = {}


def load_data(files):
    """One parse per file for the whole session (never modified)."""
    key = (files["train"], files["test"])
    if key not in _DATA:
        _DATA[key] = (vbfm.DataSubset.load(files["train"]), vbfm.DataSubset.load(files["test"]))
    return _DATA[key]


def make_learner(trace, train, test, layout="auto", rng=vbfm.RNG_REFERENCE, task="c"):
    m = trace["meta"]
    k0, k1, k = m["dim"]
    D = vbfm.num_all_attribute(train, test)
    fml = vbfm.FMLearnMCMC(k0, k1, k, D, min_target=train.min_target, max_target=train.max_target,
                           method=m["method"], layout=layout, task=task)
    fml.init(m["seed"], m["init_stdev"], regular=m["regular"], rng=rng)
    return fml


def close(a, b, rel=PRINT_REL):
    return abs(a - b) <= rel * abs(b)


CHAIN = [(c, s, l) for c in CASES for s in ("fused", "split") for l in ("auto", "column")
         if l == "auto" or c.startswith("cls_sa")]


@pytest.mark.parametrize("case,split,layout", CHAIN)
def test_chain_vs_reference(case, split, layout, cls_files, monkeypatch):
    """Per iteration the correct counts exactly and alpha, ll_mcmc_this and the hyper-priors of the
    reference's rlog to 6e-6; then the -out predictions. split: the row-sharded kernels on one rank
    (the reference stream stays usable: there is one rank); cls_sa's two one-hot fields make complete
    levels, so layout auto runs the level-ordered store."""
    if split == "split":
        monkeypatch.setenv("VBFM_FORCE_SPLIT", "1")
    monkeypatch.setenv("VBFM_LAYOUT", layout)
    t = cr.load_trace(case)
    m = t["meta"]
    train, test = load_data(cls_files(t))
    assert (train.num_cases, test.num_cases) == (m["n_train"], m["n_test"])
    fml = make_learner(t, train, test, layout)
    fml.set_data(train, test)
    fml.init_caches()
    if case.startswith("cls_sa"):
        assert fml.layout() == ("level" if layout == "auto" else "column")
    if case.startswith("cls_tiny_dup"):
        assert fml.layout() == "column"
    k = m["dim"][2]
    for it, ref in enumerate(t["iters"]):
        st = fml.iterate()
        ci = fml.class_info()
        p = fml.get_params()
        r = ref["rlog"]
        print(it, ci, st.alpha)
        assert st.rng_skipped == 0 and ci["nonfinite_rows"] == 0 and ci["capped_rows"] == 0
        assert st.train_rmse == 0 and st.rmse_all == 0 and st.rmse_this == 0 and st.mae_all == 0
        assert ci["n_train_correct"] == round(ref["train_acc"] * m["n_train"]), (it, ci, ref)
        assert ci["n_test_correct_all"] == round(ref["test_acc"] * m["n_test"]), (it, ci, ref)
        assert ci["n_test_correct_this"] == round(r["acc_mcmc_this"] * m["n_test"]), (it, ci, ref)
        assert close(ci["acc_train"], ref["train_acc"]) and close(ci["acc_all"], r["acc_mcmc_all"])
        assert close(st.alpha, r["alpha"]), (it, st.alpha, r["alpha"])
        assert close(ci["ll_this"], r["ll_mcmc_this"]), (it, ci["ll_this"], r["ll_mcmc_this"])
        assert close(p["w_mu"][0], r["wmu[0]"]) and close(p["w_lambda"][0], r["wlambda[0]"]), (it, p["w_mu"], r)
        for f in range(k):
            assert close(p["v_mu"][f], r["vmu[0,%d]" % f]), (it, f, p["v_mu"][f], r["vmu[0,%d]" % f])
            assert close(p["v_lambda"][f], r["vlambda[0,%d]" % f]), (it, f)
        # ll_all, which the reference leaves uninitialised: computed on the running mean
        assert math.isfinite(ci["ll_all"]) and ci["ll_all"] > 0
    pred = fml.predict()
    ref_pred = np.asarray(t["pred"])
    assert pred.min() >= 0.0 and pred.max() <= 1.0
    err = np.max(np.abs(pred - ref_pred) / np.abs(ref_pred))
    print("max relative difference of the predictions", err)
    assert err <= PRINT_REL
    fml.close()


def test_als_row_step_is_the_truncated_expectation(cls_files):
    """After one iteration of cls_sa/als_reg: yhat of the train rows from a snapshot of the model
    (clip = 0: the raw yhat) and e from the row caches; yhat - e is the NumPy expectation to 1e-9 on
    the rows with |yhat| <= 3, which are at least 99 % of the set."""
    t = cr.load_trace("cls_sa/als_reg")
    train, test = load_data(cls_files(t))
    fml = make_learner(t, train, test)
    fml.set_data(train, test)
    fml.init_caches()
    fml.iterate()
    ci = fml.class_info()
    model = vbfm.Model.from_learner(fml)
    assert model.task == "c"
    yhat = model.score_device(fml, 0, clip=False)
    e = fml.rows()["e"]
    y = train.target
    ok = np.abs(yhat) <= 3.0
    assert ok.mean() >= 0.99, ok.mean()
    s, want = (yhat - e)[ok], cr.expect_target(yhat[ok], y[ok])
    err = np.max(np.abs(s - want) / np.maximum(1.0, np.abs(want)))
    print("rows within |yhat| <= 3:", ok.mean(), "max difference", err)
    assert err <= 1e-9
    assert ci["n_train_correct"] == int(np.sum(cr.correct(cr.Phi(yhat), y)))
    model.close()
    fml.close()


def test_zero_target_is_sampled_as_positive_and_never_correct():
    """A hand-made set with one target-0 row: its latent target is the left expectation (y >= 0) and
    it is not counted correct whatever its prediction."""
    rng = np.random.default_rng(8)
    n, nf = 40, 6
    feat = np.stack([rng.integers(0, 3, n), 3 + rng.integers(0, 3, n)], axis=1).astype(np.uint32).ravel()
    rp = (2 * np.arange(n + 1)).astype(np.uint64)
    y = np.where(rng.random(n) < 0.5, 1.0, -1.0).astype(np.float32)
    y[17] = 0.0
    train = vbfm.DataSubset.from_csr(rp, feat, np.ones(2 * n, np.float32), y, nf)
    test = vbfm.DataSubset.from_csr(rp[:9], feat[:16], np.ones(16, np.float32), y[:8], nf)
    fml = vbfm.FMLearnMCMC(1, 1, 2, nf + 1, min_target=-1.0, max_target=1.0, method="als", task="c")
    fml.init(3, 0.1, regular=(0.5, 1.0, 2.0))
    fml.set_data(train, test)
    fml.init_caches()
    fml.iterate()
    model = vbfm.Model.from_learner(fml)
    yhat = model.score_device(fml, 0, clip=False)
    s = yhat - fml.rows()["e"]
    assert abs(s[17] - cr.expect_left(yhat[17])) <= 1e-9 and s[17] > 0
    assert abs(yhat[17]) > 1e-12        # (its side is not decided by rounding)
    others = np.arange(n) != 17
    assert fml.class_info()["n_train_correct"] == int(np.sum(cr.correct(cr.Phi(yhat[others]), y[others])))
    model.close()
    fml.close()


# ---- device mode: the latent targets drawn in the kernel ---------------------------------------
SYN = dict(rows=200_000, fields=3, ids=50, test_rows=2000)


def synth_learner(layout="auto", rows=SYN["rows"], seed=9):
    D = SYN["fields"] * SYN["ids"] + 1
    fml = vbfm.FMLearnMCMC(1, 1, 2, D, min_target=-1.0, max_target=1.0, method="mcmc", layout=layout, task="c")
    fml.init_device(seed, 0.1)
    fml.synth(0, rows, SYN["fields"], SYN["ids"], 31)
    fml.synth(1, SYN["test_rows"], SYN["fields"], SYN["ids"], 32)
    pos = fml.synth_binarize(0, 3.0)
    fml.synth_binarize(1, 3.0)
    assert 0 < pos < rows
    return fml, pos


def synth_run(iters, monkeypatch, split):
    monkeypatch.setenv("VBFM_FORCE_SPLIT", "1" if split else "0")
    fml, pos = synth_learner()
    fml.init_caches()
    out = []
    for _ in range(iters):
        st = fml.iterate()
        ci = fml.class_info()
        assert ci["nonfinite_rows"] == 0 and ci["capped_rows"] == 0
        out.append((st.alpha, st.w0, ci["n_train_correct"], ci["n_test_correct_all"], ci["ll_this"], ci["ll_all"]))
    p = fml.get_params()
    res = {"stats": out, "v": p["v"].copy(), "w": p["w"].copy(), "e": fml.rows()["e"].copy(), "pos": pos}
    fml.close()
    return res


def test_device_mode_is_deterministic_and_fused_equals_split(monkeypatch):
    """The row draws are keyed (seed, iteration, global row, attempt): a second run and the
    row-sharded kernels give the same chain bit for bit. Accuracy rises on this planted-model data."""
    a = synth_run(5, monkeypatch, False)
    b = synth_run(5, monkeypatch, False)
    c = synth_run(5, monkeypatch, True)
    for other in (b, c):
        assert a["stats"] == other["stats"]
        for key in ("v", "w", "e"):
            np.testing.assert_array_equal(a[key], other[key])
    acc = [s[2] for s in a["stats"]]
    print("train correct per iteration", acc, "positives", a["pos"])
    assert acc[-1] > acc[0]


def test_device_mode_draws_follow_the_truncated_normal():
    """After one iteration s = yhat - e lies on the target's side of 0 on every row, and the
    standardised residual (s - E[s | yhat]) / sd[s | yhat], pooled over the rows, has a mean within 5
    standard errors of 0 (exact truncated-normal moments, libm erfc)."""
    fml, _ = synth_learner()
    fml.init_caches()
    fml.iterate()
    model = vbfm.Model.from_learner(fml)
    yhat = model.score_device(fml, 0, clip=False)
    s = yhat - fml.rows()["e"]
    y = fml.get_csc(0)[2]
    assert len(y) == len(s) and set(np.unique(y)) == {-1.0, 1.0}
    pos = y >= 0
    assert np.all(s[pos] >= 0) and np.all(s[~pos] <= 0)
    # mirror the negative rows: -s is N(-yhat, 1) truncated to [0, inf)
    mu = np.where(pos, yhat, -yhat)
    z = np.where(pos, s, -s)
    erfc = np.vectorize(math.erfc)
    tail = 0.5 * erfc(-mu / math.sqrt(2.0))
    lam = np.exp(-mu * mu / 2.0) / math.sqrt(2.0 * math.pi) / tail
    mean, var = mu + lam, 1.0 - mu * lam - lam * lam
    r = (z - mean) / np.sqrt(var)
    print("pooled standardised residual", r.mean(), "+-", 1.0 / math.sqrt(len(r)), "var", r.var())
    assert abs(r.mean()) <= 5.0 / math.sqrt(len(r))
    model.close()
    fml.close()


# ---- checkpoints -------------------------------------------------------------------------------
def _three_iterations(make, path):
    """Iteration 3 of an uninterrupted run, and of a run saved after 2 and resumed in a fresh context."""
    def snap(fml):
        st = fml.iterate()
        p = fml.get_params()
        return (st.alpha, st.w0, tuple(sorted(fml.class_info().items())), p["v"].tobytes(), p["w"].tobytes(),
                p["v_lambda"].tobytes(), fml.rows()["e"].tobytes(), fml.predict().tobytes())
    a = make()
    a.init_caches()
    a.iterate()
    a.iterate()
    a.save_state(path)
    whole = snap(a)
    a.close()
    b = make()
    assert b.load_state(path) == 2
    resumed = snap(b)
    b.close()
    return whole, resumed


def test_checkpoint_resumes_the_reference_stream_chain(cls_files, tmp_path):
    t = cr.load_trace("cls_tiny/mcmc")
    train, test = load_data(cls_files(t))

    def make(task="c"):
        fml = make_learner(t, train, test, task=task)
        fml.set_data(train, test)
        return fml
    path = str(tmp_path / "chain.ckpt")
    whole, resumed = _three_iterations(make, path)
    assert whole == resumed
    r = make(task="r")
    with pytest.raises(vbfm.VbfmError, match="another task"):
        r.load_state(path)
    r.close()


def test_checkpoint_resumes_the_device_mode_chain(tmp_path):
    whole, resumed = _three_iterations(lambda: synth_learner(rows=20_000)[0], str(tmp_path / "dev.ckpt"))
    assert whole == resumed


# ---- task c is the MCMC / ALS learner's ----------------------------------------------------------
def test_vb_entry_points_refuse_a_classification_context(cls_files):
    t = cr.load_trace("cls_tiny/mcmc")
    train, test = load_data(cls_files(t))
    D = vbfm.num_all_attribute(train, test)
    fml = vbfm.FMLearnVB(1, 1, 2, D, min_target=-1.0, max_target=1.0, task="c")
    fml.init(3, 0.1)
    fml.set_data(train, test)
    for call in (fml.init_caches, fml.iterate, fml.step_w0, fml.step_w, lambda: fml.step_v(0), fml.step_hyper):
        with pytest.raises(vbfm.VbfmError, match="provided by the mcmc and als learners"):
            call()
    fml.close()
    ov = vbfm.FMLearnVBOnline(1, 1, 2, vbfm.num_all_attribute_online(train, test), min_target=-1.0, max_target=1.0,
                              task="c")
    ov.set_data(train, test)
    with pytest.raises(vbfm.VbfmError, match="provided by the mcmc and als learners"):
        ov.init(3, 0.1, num_batch=2)
    ov.close()
    reg = make_learner(t, train, test, task="r")
    with pytest.raises(vbfm.VbfmError, match="regression context"):
        reg.class_info()
    reg.close()


# ---- scoring and the CLI -------------------------------------------------------------------------
def test_saved_model_scores_probabilities(cls_files, tmp_path):
    """A task-c model saved and loaded: clip = 1 scores are Phi(clip = 0 scores) bit for bit, and on
    the fixture's test set they are pred_this of the als run.

    Phi here is the library's own link on the device. The als learner applies it to its test
    predictions (pred_this = Phi(e_test), k_mc_class_test_update), and the score kernels reproduce
    e_test bit for bit, so both halves are checked without a second implementation: clip = 0 scores
    == e_test and clip = 1 scores == pred_this, byte for byte. A NumPy Phi of the same values differs
    from the device's in the last bit of one value in eight (5.6e-17: libm's exp and the device's
    differ by an ulp), so it is held to 2 ulp of 1, not to bit equality."""
    t = cr.load_trace("cls_tiny/als_reg")
    train, test = load_data(cls_files(t))
    fml = make_learner(t, train, test)
    for _ in fml.learn(train, test, t["meta"]["iter"]):
        pass
    path = str(tmp_path / "m.vbfm")
    fml.save_model(path)
    assert vbfm.Model.file_task(path) == "c"
    m = vbfm.Model.load(path)
    assert m.task == "c" and m.info["kind"] == 2
    raw, prob = m.score(test, clip=False), m.score(test, clip=True)
    pred_this = fml.predict()
    print("raw", raw, "prob", prob, "Phi(raw) - prob", cr.Phi(raw) - prob)
    assert raw.tobytes() == fml.test_e().tobytes()
    assert prob.tobytes() == pred_this.tobytes()
    assert np.max(np.abs(prob - pred_this)) <= 1e-12
    assert np.max(np.abs(prob - cr.Phi(raw))) <= 2 * np.finfo(np.float64).eps
    assert np.max(np.abs(raw)) > 0.1 and not np.array_equal(raw, prob)
    with pytest.raises(vbfm.VbfmError, match="no variances"):
        m.score(test, variance=True)
    m.close()
    fml.close()


def _cli(cwd, *args):
    return subprocess.run([CLI] + list(args), cwd=str(cwd), capture_output=True, text=True, timeout=300)


@pytest.mark.skipif(not os.path.exists(CLI), reason="bin/libFM not built")
def test_cli_end_to_end(cls_files, tmp_path):
    """bin/libFM -task c on cls_tiny: the "#Iter=" lines, -out, -rlog and -save_model, then
    -load_model (the task comes from the file; a contradicting -task is refused)."""
    import re
    t = cr.load_trace("cls_tiny/mcmc")
    m = t["meta"]
    f = cls_files(t)
    r = _cli(tmp_path, "-task", "c", "-train", f["train"], "-test", f["test"], "-method", "mcmc", "-dim",
             ",".join(str(x) for x in m["dim"]), "-iter", str(m["iter"]), "-seed", str(m["seed"]), "-out", "pred.txt",
             "-rlog", "rlog.tsv", "-save_model", "m.vbfm", "-vfile", "0")
    assert "ERROR" not in r.stderr, r.stderr
    lines = re.findall(r"#Iter=\s*(\d+)\tTrain=(\S+)\tTest=(\S+)", r.stdout)
    assert len(lines) == m["iter"] and "MAP@" not in r.stdout
    for (it, tr_acc, te_acc), ref in zip(lines, t["iters"]):
        assert int(it) == ref["iter"] and close(float(tr_acc), ref["train_acc"]) and close(float(te_acc), ref["test_acc"])
    pred = np.loadtxt(str(tmp_path / "pred.txt"))
    assert np.max(np.abs(pred - np.asarray(t["pred"])) / np.asarray(t["pred"])) <= 2 * PRINT_REL   # both print 6 digits
    with open(str(tmp_path / "rlog.tsv")) as fh:
        head = fh.readline().rstrip("\n").split("\t")
        rows = [dict(zip(head, (float(x) for x in ln.split("\t")))) for ln in fh if ln.strip()]
    assert head[:12] == ["accuracy", "time_pred", "time_learn", "time_learn2", "time_learn4", "alpha", "acc_mcmc_this",
                         "acc_mcmc_all", "acc_mcmc_all_but5", "ll_mcmc_this", "ll_mcmc_all", "ll_mcmc_all_but5"]
    for row, ref in zip(rows, t["iters"]):
        for key, v in ref["rlog"].items():
            assert close(row[key], v, 2 * PRINT_REL), (key, row[key], v)
        assert row["acc_mcmc_all_but5"] == 0 and row["ll_mcmc_all_but5"] == 0 and row["ll_mcmc_all"] > 0
    s = _cli(tmp_path, "-load_model", "m.vbfm", "-test", f["test"], "-out", "scored.txt")
    assert "ERROR" not in s.stderr and "task c" in s.stdout and "Test accuracy=" in s.stdout, s.stdout + s.stderr
    scored = np.loadtxt(str(tmp_path / "scored.txt"))
    assert len(scored) == m["n_test"] and scored.min() >= 0 and scored.max() <= 1
    s = _cli(tmp_path, "-task", "c", "-load_model", "m.vbfm", "-test", f["test"], "-out", "scored_c.txt")
    assert "ERROR" not in s.stderr and os.path.exists(str(tmp_path / "scored_c.txt"))
    s = _cli(tmp_path, "-task", "r", "-load_model", "m.vbfm", "-test", f["test"], "-out", "scored_r.txt")
    assert "ERROR: -task r contradicts the model file" in s.stderr and not os.path.exists(str(tmp_path / "scored_r.txt"))


def _zero_one(src, dst):
    """The same file with the negative class labelled 0 instead of -1."""
    with open(src) as fi, open(dst, "w") as fo:
        for line in fi:
            fo.write("0" + line[2:] if line.startswith("-1") else line)


@pytest.mark.skipif(not os.path.exists(CLI), reason="bin/libFM not built")
def test_cli_maps_zero_one_labels_like_the_reference(cls_files, tmp_path):
    """libfm.cpp:339-340: the classes are target <= 0 and target > 0. Files labelled 0 / 1 train the
    chain of the -1 / +1 files, the saved model records the mapped range, and -load_model counts a
    0-labelled test row as the negative class."""
    import re
    t = cr.load_trace("cls_tiny/als_reg")
    m = t["meta"]
    f = cls_files(t)
    tr01, te01 = str(tmp_path / "train01.libfm"), str(tmp_path / "test01.libfm")
    _zero_one(f["train"], tr01)
    _zero_one(f["test"], te01)
    assert any(l.startswith("0 ") for l in open(te01))
    r = _cli(tmp_path, "-task", "c", "-train", tr01, "-test", te01, "-method", "als", "-dim",
             ",".join(str(x) for x in m["dim"]), "-iter", str(m["iter"]), "-seed", str(m["seed"]), "-regular",
             ",".join(str(x) for x in m["regular"]), "-save_model", "m.vbfm", "-vfile", "0")
    assert "ERROR" not in r.stderr, r.stderr
    lines = re.findall(r"#Iter=\s*(\d+)\tTrain=(\S+)\tTest=(\S+)", r.stdout)
    assert len(lines) == m["iter"]
    for (it, tr_acc, te_acc), ref in zip(lines, t["iters"]):
        assert close(float(tr_acc), ref["train_acc"]) and close(float(te_acc), ref["test_acc"])
    info = vbfm.Model.file_info(str(tmp_path / "m.vbfm"))
    assert (info["min_target"], info["max_target"]) == (-1.0, 1.0)
    acc = []
    for te in (te01, f["test"]):
        s = _cli(tmp_path, "-load_model", "m.vbfm", "-test", te, "-out", "scored.txt")
        assert "ERROR" not in s.stderr, s.stderr
        acc.append(re.search(r"Test accuracy=(\S+)", s.stdout).group(1))
    # als: -out / pred_this of the last iteration are what the saved model scores
    assert acc[0] == acc[1] and close(float(acc[0]), t["iters"][-1]["rlog"]["acc_mcmc_this"])


def test_a_larger_train_set_in_the_same_context(cls_files):
    """The buffer of the latent targets drawn from the reference stream follows the train set: a
    context that trained on 1,000 rows takes the whole 90,000-row set next, and every one of its rows
    gets a target on its own side of 0."""
    t = cr.load_trace("cls_sa/mcmc")
    train, test = load_data(cls_files(t))
    fml = make_learner(t, train, test)
    for part in (_shard(train, 0, 1000), train):
        fml.set_data(part, test)
        fml.init_caches()
        fml.iterate()
        ci = fml.class_info()
        assert ci["nonfinite_rows"] == 0 and 0 < ci["n_train_correct"] <= part.num_cases
        model = vbfm.Model.from_learner(fml)
        s = model.score_device(fml, 0, clip=False) - fml.rows()["e"]
        model.close()
        assert len(s) == part.num_cases
        pos = part.target >= 0
        assert np.all(s[pos] >= 0) and np.all(s[~pos] <= 0) and np.all(s != 0)
    fml.close()


def test_binarize_under_row_caches_asks_for_them_again():
    """vbfm_synth_binarize rewrites the train targets: the row caches of the old targets are dropped."""
    fml, _ = synth_learner(rows=5000)
    fml.init_caches()
    fml.iterate()
    fml.synth_binarize(0, 4.0)     # (already -1 / +1: every row turns negative)
    with pytest.raises(vbfm.VbfmError, match="vbfm_mcmc_init_caches first"):
        fml.iterate()
    fml.init_caches()
    fml.iterate()
    assert fml.class_info()["nonfinite_rows"] == 0
    fml.close()


# ---- row shards: 2 ranks on one GPU through the host exchange ---------------------------------------
def _shard(ds, lo, hi):
    rp = ds.row_ptr.astype(np.int64)
    sl = slice(int(rp[lo]), int(rp[hi]))
    return vbfm.DataSubset.from_csr((rp[lo:hi + 1] - rp[lo]).astype(np.uint64), ds.row_ent["id"][sl],
                                    ds.row_ent["value"][sl], ds.target[lo:hi], ds.num_feature)


def _shard_run(fml, train, test, iters):
    fml.set_data(train, test)
    fml.init_caches()
    out = []
    for _ in range(iters):
        st = fml.iterate()
        ci = fml.class_info()
        out.append((ci["n_train_correct"], ci["n_test_correct_this"], ci["n_test_correct_all"], ci["ll_this"],
                    ci["ll_all"], st.alpha, ci["nonfinite_rows"], ci["capped_rows"]))
    p = fml.get_params()
    return {"stats": out, "v": p["v"], "w": p["w"]}


def _shard_worker(rank, world, store_path, files, method, rng, iters, out_q):
    try:
        import torch
        import torch.distributed as dist
        # the rendezvous is a file the parent made: no port is picked, released and reused
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
        D = vbfm.num_all_attribute(train, test)

        def learner():
            fml = vbfm.FMLearnMCMC(1, 1, 8, D, min_target=-1.0, max_target=1.0, method=method, task="c")
            fml.init(42, 0.1, regular=(0.0, 1.0, 5.0) if method == "als" else (), rng=rng)
            return fml
        fml = learner()
        fml.comm_init_host(world, rank, allreduce)
        msg = {}
        try:
            msg["sharded"] = _shard_run(fml, _shard(train, rank * N // world, (rank + 1) * N // world),
                                        _shard(test, rank * Nt // world, (rank + 1) * Nt // world), iters)
        except vbfm.VbfmError as exc:
            msg["refused"] = str(exc)
        fml.close()
        if rank == 0:
            if "sharded" in msg:
                ref = learner()
                msg["single"] = _shard_run(ref, train, test, iters)
                ref.close()
            out_q.put(msg)
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as exc:   # reported to the parent instead of a silent hang
        import traceback
        out_q.put({"error": "rank %d: %r\n%s" % (rank, exc, traceback.format_exc())})


def _launch(files, method, rng, iters, tmp_path):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    store_path = str(tmp_path / "rendezvous")
    procs = [ctx.Process(target=_shard_worker, args=(r, 2, store_path, files, method, rng, iters, q)) for r in range(2)]
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
    return msg


@pytest.mark.parametrize("method,rng", [("als", vbfm.RNG_REFERENCE), ("mcmc", vbfm.RNG_DEVICE)])
def test_row_shards_match_one_rank(method, rng, cls_files, tmp_path):
    """cls_sa on 2 ranks (contiguous row shards; the device draws are keyed by the global row) vs one
    rank: equal correct counts, parameters to 1e-9."""
    msg = _launch(cls_files(cr.load_trace("cls_sa/mcmc")), method, rng, 2, tmp_path)
    s, r = msg["sharded"], msg["single"]
    for a, b in zip(s["stats"], r["stats"]):
        print(a, b)
        assert a[:3] == b[:3] and a[6:] == b[6:] == (0, 0)
        for x, y in zip(a[3:6], b[3:6]):
            assert abs(x - y) <= 1e-9 * abs(y)
    for key in ("v", "w"):
        err = np.max(np.abs(s[key] - r[key])) / np.max(np.abs(r[key]))
        print(key, err)
        assert err <= 1e-9


def test_reference_stream_sampling_on_two_ranks_is_refused(cls_files, tmp_path):
    msg = _launch(cls_files(cr.load_trace("cls_tiny/mcmc")), "mcmc", vbfm.RNG_REFERENCE, 1, tmp_path)
    assert "refused" in msg and "needs VBFM_RNG_DEVICE" in msg["refused"], msg

"""The device-RNG (VBFM_RNG_DEVICE) chains of the MCMC / ALS learner held to the CPU oracle draw for
draw, where tests/test_mcmc_gpu.py and tests/test_class_gpu.py only ask them to be deterministic
and statistically plausible.

The oracle (oracle/vbfm_oracle.c) starts from the parameters the device initialised, takes alpha,
w0 and the hyper-prior draws from the srand(seed) stream as the library does, and the per-attribute
normals and task c's latent targets from tests/keyed_rng.py, the NumPy restatement of the documented
keying (include/vbfm.h). tests/test_device_rng_cpu.py pins that restatement to the library's header
compiled for the host, the oracle's task c to the compiled reference, and shows that every chain
here is stable under a change of the normals larger than the device's libm can make. So the bound
is REL, tests/test_mcmc_gpu.py's bound for the same data on the reference stream: a wrong key, a
shared stream, a draw in the wrong record or another branch of the sampler differs by O(1).
"""
import os

import numpy as np
import pytest

import device_rng_cases as dc
import keyed_rng as kr
import vbfm
from conftest import GOLDEN
from test_mcmc_gpu import REL

pytestmark = pytest.mark.gpu

INIT_TOL = 1e-14     # |x - init_stdev * normal| <= INIT_TOL * max(1, |x|): a wrong key differs by O(init_stdev)
# |s - restatement| <= DRAW_TOL * max(1, |s|). Derived: the device's log, sqrt, cos and exp are within
# 2 ulp and |z| <= 8.6 for 53-bit uniforms, so a correct draw differs by less than 2e-14; a wrong key,
# branch or record differs by O(1).
DRAW_TOL = 1e-12

FORMS = {"fused": {"VBFM_FORCE_SPLIT": "0"}, "split": {"VBFM_FORCE_SPLIT": "1"},
         "two-pass": {"VBFM_FORCE_SPLIT": "1", "VBFM_DEFER": "0"}}
LAYOUT_OF = {"tiny": "entry", "tiny_dup": "column"}   # what auto picks; synth / syn: the level store


@pytest.fixture(scope="module")
def cls_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("cls_device_rng")


def set_env(monkeypatch, layout, form):
    for name in ("VBFM_DEFER", "VBFM_PREDICT", "VBFM_MC_FUSED_PREDICT", "VBFM_FORCE_SPLIT"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("VBFM_LAYOUT", layout)
    for name, value in FORMS[form].items():
        monkeypatch.setenv(name, value)


@pytest.fixture(scope="module")
def shared():
    """What the tests of this module compute once and only read afterwards: the data sets by
    (data, threshold) and the oracle's chains by case. Both end with the module."""
    return {"data": {}, "oracle": {}}


def data_of(shared, case, cls_dir, synth_files):
    """The case's (train, test) for the library and for the oracle, made once and never modified."""
    key = (case.data, case.threshold)
    if key not in shared["data"]:
        src = dc.sources(case, cls_dir, synth_files)
        nf = dc.SYN["fields"] * dc.SYN["ids"]
        dev = tuple(vbfm.DataSubset.load(s) if isinstance(s, str) else vbfm.DataSubset.from_csr(*s[1:], nf) for s in src)
        shared["data"][key] = (dev, dc.oracle_data(src))
    return shared["data"][key]


def make_learner(case, train, test, layout="auto"):
    k0, k1, k = case.dim
    D = vbfm.num_all_attribute(train, test)
    groups = None if case.meta is None else vbfm.load_meta(os.path.join(GOLDEN, case.data, case.meta), D)
    fml = vbfm.FMLearnMCMC(k0, k1, k, D, attr_group=groups, min_target=train.min_target, max_target=train.max_target,
                           method=case.method, layout=layout, task=case.task)
    fml.init(case.seed, case.init_stdev, regular=case.regular,
             rng=vbfm.RNG_DEVICE if case.rng == "device" else vbfm.RNG_REFERENCE)
    return fml


def expected_layout(case, layout):
    if layout != "auto":
        return layout
    return LAYOUT_OF.get(case.data, "level")


def oracle_of(shared, case, otrain, otest, start):
    """The oracle's chain of a case, computed once: the start is the device's own initialisation,
    which must be the same, value for value, for every layout and form that reuses the chain."""
    cache = shared["oracle"]
    if case.name not in cache:
        snaps, o = dc.oracle_chain(case, otrain, otest, start=start)
        cache[case.name] = (start, snaps, o.predict())
    kept = cache[case.name][0]
    assert (start is None) == (kept is None)
    if start is not None:
        assert set(start) == set(kept)
        for key in start:
            np.testing.assert_array_equal(np.asarray(start[key]), np.asarray(kept[key]), err_msg=key)
    return cache[case.name][1:]


def snapshot(fml, st, task):
    s = fml.get_params()
    s["e"] = fml.rows()["e"]
    if task == "c":
        s.update(fml.class_info())
    else:
        s.update(rmse_all=st.rmse_all, rmse_this=st.rmse_this, train_rmse=st.train_rmse)
    return s


CHAINS = [(c, l, f) for c in dc.REGRESSION + dc.CLASSIFICATION if c.name not in dc.DROPPED for l in c.layouts
          for f in (("fused", "split", "two-pass") if l == "level" else ("fused", "split"))]


@pytest.mark.parametrize("case,layout,form", CHAINS, ids=lambda x: str(x))
def test_chain_vs_oracle(case, layout, form, shared, cls_dir, synth_files, monkeypatch):
    """After every iteration w, v, the hyper-priors, alpha, w0, the row caches e and the iteration's
    figures (regression: rmse_all, rmse_this, train_rmse; task c: ll_this, ll_all, and the three
    correct counts exactly) against the oracle's to REL; at the end predict(). Fused and row-sharded
    split kernels (on the level store also the two-pass form), every layout of the case. The als
    cases of task c run on the reference stream and hold its chain to REL instead of six digits."""
    set_env(monkeypatch, layout, form)
    (train, test), (otrain, otest) = data_of(shared, case, cls_dir, synth_files)
    fml = make_learner(case, train, test, layout)
    start = None
    if case.rng == "device":
        start = {k: v for k, v in fml.get_params().items() if k != "reg0"}
    want, want_pred = oracle_of(shared, case, otrain, otest, start)
    fml.set_data(train, test)
    fml.init_caches()
    if case.dim[2] >= 2:
        assert fml.layout() == expected_layout(case, layout)
    worst = {}
    for it in range(case.iters):
        st = fml.iterate()
        assert st.rng_skipped == 0
        if case.task == "c":
            ci = fml.class_info()
            assert ci["nonfinite_rows"] == 0 and ci["capped_rows"] == 0
        dc.compare(case.task, snapshot(fml, st, case.task), want[it], worst, REL)   # asserts per quantity, NaN-safe
        assert max(worst.values()) <= REL, (case, it, worst)
    worst["predict"] = dc.rel_err(fml.predict(), want_pred)
    print("FIG chain", case, layout, form, " ".join("%s=%.1e" % kv for kv in sorted(worst.items())))
    assert worst["predict"] <= REL
    fml.close()


@pytest.mark.parametrize("k,D,seed,stdev", [(3, 27, 5, 0.1), (4, 2001, 7, 0.1), (0, 27, 5, 0.1), (1, 300, 11, 0.2),
                                             (2, 151, 20261021, 0.1)])
def test_initialisation_is_the_documented_streams(k, D, seed, stdev):
    """vbfm_mcmc_init in device mode, before any iteration: w[j] = init_stdev * normal(seed,
    bit 62 | 22, j) and v_f[j] = init_stdev * normal(seed, bit 62 | 21, j * k + f), which pins the
    index order of the pair store as well; the hyper-priors, w0 and alpha of fm_learn_mcmc::init."""
    fml = vbfm.FMLearnMCMC(1, 1, k, D, method="mcmc")
    fml.init(seed, stdev, rng=vbfm.RNG_DEVICE)
    p = fml.get_params()
    fml.close()
    w, v = kr.init_params(seed, stdev, k, D)
    worst = 0.0
    for got, want in ((p["w"], w), (p["v"], v)):
        assert got.shape == want.shape
        assert np.isfinite(got).all() and np.isfinite(want).all()
        if want.size:
            err = float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))
            assert err <= INIT_TOL, err
            worst = max(worst, err)
            assert np.std(got) > 0.5 * stdev
    print("FIG init k=%d D=%d %.1e" % (k, D, worst))
    assert worst <= INIT_TOL
    assert p["w0"] == 0.0 and p["alpha"] == 1.0
    for key in ("w_mu", "w_lambda", "v_mu", "v_lambda"):
        assert not p[key].any()


def latent_targets(fml):
    """yhat of the train rows from a snapshot of the model (clip = 0: the raw yhat) and the latent
    target s = yhat - e the row step left."""
    model = vbfm.Model.from_learner(fml)
    yhat = model.score_device(fml, 0, clip=False)
    model.close()
    return yhat, yhat - fml.rows()["e"]


def check_draws(tag, fml, case, it, y):
    yhat, s = latent_targets(fml)
    want, attempts, flag, dist = kr.class_sample_target(yhat, y >= 0, case.seed, kr.CLASS_STREAM | it, np.arange(len(y)))
    ci = fml.class_info()
    assert ci["capped_rows"] == 0 and ci["nonfinite_rows"] == 0 and not flag.any()
    assert dist.min() > dc.MIN_DIST, dist.min()
    assert np.isfinite(s).all() and np.isfinite(want).all() and np.isfinite(yhat).all()
    err = float(np.max(np.abs(s - want) / np.maximum(1.0, np.abs(want))))
    robert = np.where(y >= 0, -yhat, yhat) > 0
    print("FIG draws", tag, "iteration", it, "max difference %.1e" % err, "closest decision %.1e" % dist.min(),
          "rows in Robert's branch", int(robert.sum()), "attempts up to", int(attempts.max()))
    assert err <= DRAW_TOL
    return yhat, s, robert


@pytest.mark.parametrize("layout", ["auto", "column"])
def test_latent_draws_row_by_row(layout, shared, cls_dir, monkeypatch):
    """Task c on the 5,000-row set: after each of three iterations every row's latent target is the
    restatement's draw for key (seed, bit 63 | iteration, row) on that row's yhat, to DRAW_TOL; no
    row decides within 1e-9 of a boundary, so none is excluded. The three iterations draw different
    noise. Then w0 = +4 and w0 = -4 through set_params, one iteration each: the rows whose target
    disagrees with the sign of yhat enter Robert's branch with left of about 4."""
    set_env(monkeypatch, layout, "fused")
    case = dc.by_name("syn5000/mcmc")
    (train, test), _ = data_of(shared, case, cls_dir, None)
    fml = make_learner(case, train, test, layout)
    fml.set_data(train, test)
    fml.init_caches()
    assert fml.layout() == expected_layout(case, layout)
    y = train.target
    noise = []
    for it in range(3):
        fml.iterate()
        yhat, s, _ = check_draws(layout, fml, case, it, y)
        noise.append(np.abs(s - yhat))
    for a in range(3):
        for b in range(a + 1, 3):
            assert np.mean(np.abs(noise[a] - noise[b]) > 1e-3) > 0.9
    for it, w0 in ((3, 4.0), (4, -4.0)):
        fml.set_params({"w0": w0})
        fml.iterate()
        yhat, _, robert = check_draws("%s w0=%+g" % (layout, w0), fml, case, it, y)
        deep = robert & (np.abs(yhat) > 2.0)
        assert robert.sum() >= 1000 and deep.sum() >= 1000, (robert.sum(), deep.sum())
    fml.close()


@pytest.mark.parametrize("layout", ["auto", "column"])
def test_nonfinite_rows_are_counted(layout, shared, cls_dir, monkeypatch):
    """w[j] = +inf for one attribute: its draw is refused (the reference restores the old value), the
    m rows that contain j predict a non-finite yhat, and the row step counts exactly those."""
    set_env(monkeypatch, layout, "fused")
    case = dc.by_name("syn5000/mcmc")
    (train, test), _ = data_of(shared, case, cls_dir, None)
    fml = make_learner(case, train, test, layout)
    fml.set_data(train, test)
    fml.init_caches()
    j = 57
    m = int(train.col_ptr[j + 1] - train.col_ptr[j])
    assert 10 <= m < train.num_cases
    w = fml.get_params()["w"]
    w[j] = np.inf
    fml.set_params({"w": w})
    fml.iterate()
    ci = fml.class_info()
    print("rows of attribute", j, m, ci)
    assert ci["nonfinite_rows"] == m and ci["capped_rows"] == 0
    e = fml.rows()["e"]
    rows = train.col_ent["id"][int(train.col_ptr[j]):int(train.col_ptr[j + 1])]
    assert np.all(np.isnan(e[rows])) and np.isfinite(np.delete(e, rows)).all()
    fml.close()

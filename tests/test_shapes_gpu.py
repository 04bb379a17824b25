"""Every workgroup shape of the level sweeps against the CPU oracle.

A level kernel takes its shape (BLOCK threads x R records, CAP = BLOCK x R) from the level's mean
column length (dispatch_shape, csrc/vbfm_device.h; restated as synth.SHAPE_TABLE). The shape
decides the reduction tree (one wave, or several through LDS), the LDS staging, and for a column
beyond CAP the chunked path of the level store or the overflow loops of the column-gather kernels.
The other GPU tests compare with a reference almost only at 64 x 2; the larger shapes are met by
tests that compare the library with itself, or by the full-size runs.

Here every shape runs on a data set of at most 5,634 rows (tests/shape_cases.py): three one-hot
fields, each a level whose columns are CAP, CAP + 1 (streamed, a last chunk of one record),
2 CAP + 1 (three chunks), 1, CAP - 1 and CAP / 2 long, with a mean inside the shape's band. Each
test first asserts, from the learner's own levels() and CSC, that the band is the intended one,
that no column is segmented and that the layout is the requested one; tests/test_shapes_cpu.py
checks the same without a GPU.

  VB:    e, t, the last factor's q-cache, mu_w, mu_v and the free energy of three iterations at
         TOL = 1e-12 (tree against sequential column sums, as tests/test_levels_gpu.py), fused,
         two-pass split and deferred split; the forms bit-identical on the level store.
  ALS (-regular 0.5,1,2) and MCMC on the reference's random stream: Train / Test values of every
         iteration and the final parameters and hyper-parameters at REL = 1e-9 (the chain bound of
         tests/test_mcmc_gpu.py), fused and split; bit-identical draws on the level store; the
         fused train re-prediction bit-identical to the separate one.
  k = 3 everywhere (w with a next factor, both q-cache slots with one, the last factor without);
  k = 2 (slot 1 without a next factor) and k = 0 (w without one) fused on the level store and the
  column layout; x = 1 everywhere (no x array, the deferred kernels' 8-byte payload) on the level
  store at k = 3.

The oracle's own chains on these data sets move by at most 3e-15 relative under a 2-ulp
perturbation of a factor, and a lost or doubled record of a 1,024-entry column moves a statistic
by ~1e-3, so both bounds decide. Every test prints its largest error per quantity.
"""
import numpy as np
import pytest

import shape_cases as sc
import vbfm
from test_levels_gpu import TOL, _few_forms, rel_err
from test_mcmc_gpu import REL

pytestmark = pytest.mark.gpu

LAYOUTS = ["level", "column", "entry"]
VB_KEYS = ("e", "t", "q", "tq", "tz", "mu_w", "mu_v", "free_energy")
MC_KEYS = ("w", "v", "w_mu", "w_lambda", "v_mu", "v_lambda")
ENV = sc.SHAPE_ENV + ("VBFM_FORCE_SPLIT", "VBFM_DEFER", "VBFM_LX", "VBFM_PREDICT", "VBFM_MC_FUSED_PREDICT")
shapes = pytest.mark.parametrize("shape", sc.SHAPES, ids=sc.SHAPE_IDS)


def _env(monkeypatch, env):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def _sets(shape, xmode):
    tr, te, nf, nft, D = sc.data(shape, xmode)
    return vbfm.DataSubset.from_csr(*tr, nf), vbfm.DataSubset.from_csr(*te, nft), D


def _conditions(g, shape, layout, xmode):
    """Before anything is compared: the learner's levels run `shape`, whole, on `layout`."""
    lv, L = g.levels()
    cp, ent, _ = g.get_csc(0)
    sc.check_conditions(shape, lv, L, cp)
    assert g.layout() == layout
    assert bool((ent["value"] == 1).all()) == (xmode == 0)


def _vb_run(shape, layout, k, xmode, env, monkeypatch):
    _env(monkeypatch, env)
    train, test, D = _sets(shape, xmode)
    g = vbfm.FMLearnVB(1, 1, k, D, min_target=train.min_target, max_target=train.max_target, layout=layout)
    g.init(sc.SEED, sc.INIT_STDEV)
    g.set_data(train, test)
    g.init_caches()
    _conditions(g, shape, layout, xmode)
    fe = [g.iterate().free_energy for _ in range(sc.ITERS)]
    r, p = g.rows(), g.get_params()
    g.close()
    return dict(r, mu_w=np.asarray(p["mu_w"]), mu_v=np.asarray(p["mu_v"]), free_energy=np.asarray(fe))


def _vb_close(res, ref, k, what):
    errs = {key: rel_err(res[key], ref[key]) for key in VB_KEYS if not (k == 0 and key in ("q", "tq", "tz"))}
    print("vb %s:" % (what,), " ".join("%s %.2e" % kv for kv in errs.items()))
    for key, err in errs.items():
        assert err <= TOL, (what, key, err)


def _vb_forms(layout, forms):
    return [(name, env) for name, env in _few_forms(layout) if name in forms]


def _vb_case(shape, layout, k, xmode, forms, monkeypatch):
    ref = sc.oracle_vb(shape, k, xmode)
    res = {}
    for form, env in _vb_forms(layout, forms):
        res[form] = _vb_run(shape, layout, k, xmode, env, monkeypatch)
        _vb_close(res[form], ref, k, (shape, layout, "k=%d" % k, "x%d" % xmode, form))
    if layout == "level":          # one reduction tree, one order of the records: the same bits
        for form in res:
            for key in VB_KEYS:
                np.testing.assert_array_equal(res[form][key], res[forms[0]][key], err_msg="%s %s" % (form, key))


@pytest.mark.parametrize("layout", LAYOUTS)
@shapes
def test_vb_vs_oracle(shape, layout, monkeypatch):
    """k = 3, stored x: the fused sweep and both split forms against the oracle."""
    _vb_case(shape, layout, 3, 1, ("fused", "two-pass", "deferred"), monkeypatch)


@pytest.mark.parametrize("layout", ["level", "column"])
@pytest.mark.parametrize("k", [2, 0])
@shapes
def test_vb_few_factors_vs_oracle(shape, k, layout, monkeypatch):
    """The sweep variants a k = 3 run never launches: slot 1 without a next factor (k = 2), w
    without one (k = 0)."""
    _vb_case(shape, layout, k, 1, ("fused",), monkeypatch)


@shapes
def test_vb_unit_x_vs_oracle(shape, monkeypatch):
    """Every x is 1: the level store keeps no x array and the deferred kernels read their 8-byte
    payload."""
    _vb_case(shape, "level", 3, 0, ("fused", "deferred"), monkeypatch)


# ---- ALS / MCMC ------------------------------------------------------------------------------
MC_FORMS = (("fused", {"VBFM_FORCE_SPLIT": "0"}), ("split", {"VBFM_FORCE_SPLIT": "1"}))


def _mc_run(shape, method, layout, k, xmode, env, monkeypatch):
    _env(monkeypatch, env)
    train, test, D = _sets(shape, xmode)
    g = vbfm.FMLearnMCMC(1, 1, k, D, min_target=train.min_target, max_target=train.max_target, method=method,
                         layout=layout)
    g.init(sc.SEED, sc.INIT_STDEV, regular=sc.REGULAR if method == "als" else (), rng=vbfm.RNG_REFERENCE)
    g.set_data(train, test)
    g.init_caches()
    _conditions(g, shape, layout, xmode)
    stats = []
    for _ in range(sc.ITERS):
        st = g.iterate()
        assert st.rng_skipped == 0
        stats.append((st.rmse_all, st.rmse_this, st.train_rmse, st.alpha, st.w0))
    p, e = g.get_params(), g.rows()["e"]
    g.close()
    return stats, p, e


def _mc_close(res, ref, what):
    stats, p, _ = res
    trace, rp = ref
    errs = {"test": 0.0, "train": 0.0}
    for st, (rmse_all, _, train) in zip(stats, trace):
        errs["test"] = max(errs["test"], abs(st[0] - rmse_all) / rmse_all)
        errs["train"] = max(errs["train"], abs(st[2] - train) / train)
    for key in ("w0", "alpha"):
        errs[key] = abs(p[key] - rp[key]) / max(abs(rp[key]), 1e-300)
    for key in MC_KEYS:
        errs[key] = rel_err(p[key], rp[key])
    print("%s:" % (what,), " ".join("%s %.2e" % kv for kv in errs.items()))
    for key, err in errs.items():
        assert err <= REL, (what, key, err)


def _mc_case(shape, method, layout, k, xmode, forms, monkeypatch):
    ref = sc.oracle_mc(shape, method, k, xmode)
    res = {}
    for form, env in MC_FORMS:
        if form in forms:
            res[form] = _mc_run(shape, method, layout, k, xmode, env, monkeypatch)
            _mc_close(res[form], ref, (method, shape, layout, "k=%d" % k, "x%d" % xmode, form))
    if layout == "level" and len(res) == 2:      # the same statistics, so the same draws
        a, b = res["fused"], res["split"]
        assert [s[0] for s in a[0]] == [s[0] for s in b[0]]
        for key in ("w", "v"):
            np.testing.assert_array_equal(a[1][key], b[1][key], err_msg=key)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("method", ["als", "mcmc"])
@shapes
def test_mcmc_als_vs_oracle(shape, method, layout, monkeypatch):
    """k = 3, stored x: the fused sweep and the split one (deferred on the level store, two-pass
    elsewhere) follow the oracle's chain."""
    _mc_case(shape, method, layout, 3, 1, ("fused", "split"), monkeypatch)


@pytest.mark.parametrize("layout", ["level", "column"])
@pytest.mark.parametrize("k", [2, 0])
@pytest.mark.parametrize("method", ["als", "mcmc"])
@shapes
def test_mcmc_als_few_factors_vs_oracle(shape, method, k, layout, monkeypatch):
    _mc_case(shape, method, layout, k, 1, ("fused",), monkeypatch)


@pytest.mark.parametrize("method", ["als", "mcmc"])
@shapes
def test_mcmc_als_unit_x_vs_oracle(shape, method, monkeypatch):
    _mc_case(shape, method, "level", 3, 0, ("fused", "split"), monkeypatch)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("method", ["als", "mcmc"])
@shapes
def test_fused_train_prediction_is_bit_identical(shape, method, layout, monkeypatch):
    """The train re-prediction accumulated inside the v sweeps against the separate pass in the
    reference's order (VBFM_MC_FUSED_PREDICT=0): the same statistics and rows e, fused and split."""
    for split in ("0", "1"):
        out = [_mc_run(shape, method, layout, 3, 1, {"VBFM_FORCE_SPLIT": split, "VBFM_PREDICT": "exact",
                                                     "VBFM_MC_FUSED_PREDICT": fused}, monkeypatch)
               for fused in ("0", "1")]
        assert out[0][0] == out[1][0], split
        np.testing.assert_array_equal(out[0][2], out[1][2], err_msg="e, split " + split)
        np.testing.assert_array_equal(out[0][1]["v"], out[1][1]["v"], err_msg="v, split " + split)

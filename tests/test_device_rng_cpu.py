"""What entitles the CPU oracle to judge the device-mode (VBFM_RNG_DEVICE) chains, without a GPU:

- the NumPy restatement of the counter-based generator (tests/keyed_rng.py) against the library's
  own header compiled for the host (tests/class_math_check.cpp `draws`, under ASan + UBSan);
- the oracle's task c against the compiled reference's runs (tests/golden/cls_*), by
  tests/test_class_gpu.py's rules;
- every chain tests/test_device_rng_gpu.py runs is stable enough to be compared at 1e-9: two oracle
  chains whose normals differ by more than the device's libm can differ agree to 1e-11;
- no two draws of a run share a stream id.
"""
import os
import subprocess

import numpy as np
import pytest

import class_ref as cr
import device_rng_cases as dc
import keyed_rng as kr
import oracle_ctypes as oc
from test_class_cpu import check_exe, needs_gxx   # noqa: F401  (the fixture that builds class_math_check)
from test_class_gpu import PRINT_REL, close

GRID = (0.0, 1e-3, -1e-3, 0.5, -0.5, 2.0, -2.0, 4.0, -4.0, 6.0, -6.0)
ROWS_EACH = 2000


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.abs(b))


@needs_gxx
@pytest.mark.parametrize("seed,stream,row0", [(9, kr.CLASS_STREAM | 2, 0), (1792455606, kr.CLASS_STREAM, 2 ** 33 + 7)])
def test_restatement_matches_the_header(check_exe, seed, stream, row0):   # noqa: F811
    """class_sample_target on yhat in {0, +-1e-3, +-0.5, +-2, +-4, +-6}, both sides, 2,000 rows each:
    s to 4 ulp, the attempts and flags exactly; no row's decision lies within 1e-12 of its boundary,
    so none is left out. device_normal on the sweeps', the initialisation's and large stream ids."""
    yhat = np.repeat(np.array([y for y in GRID for _ in (0, 1)]), ROWS_EACH)
    side = np.tile(np.repeat(np.array([1, 0]), ROWS_EACH), len(GRID))
    n = len(yhat)
    normals = [(st, j) for st in (0, 5, 21, 22, kr.INIT_V, kr.INIT_W, 2 ** 32 + 3, 25 * 101 - 1)
               for j in (0, 1, 2, 1000, 2 ** 31, 2 ** 40 + 1)]
    text = "".join("%.17g %d\n" % (y, s) for y, s in zip(yhat, side)) + "".join("%d %d\n" % p for p in normals)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([check_exe, "draws", str(seed), str(stream), str(row0), str(n)], input=text, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == n + len(normals)
    got = np.array([[float(x) for x in ln.split()] for ln in lines[:n]])
    s, attempts, flag, dist = kr.class_sample_target(yhat, side > 0, seed, stream, row0 + np.arange(n, dtype=np.uint64))
    print("closest decision", dist.min(), "attempts up to", attempts.max(), "largest difference of s in ulp",
          ulps(s, got[:, 0]).max())
    assert np.sum(dist < 1e-12) == 0
    np.testing.assert_array_equal(attempts, got[:, 1].astype(np.int64))
    np.testing.assert_array_equal(flag, got[:, 2].astype(np.int64))
    assert not flag.any()
    assert ulps(s, got[:, 0]).max() <= 4
    pos = side > 0
    assert np.all(s[pos] >= 0) and np.all(s[~pos] <= 0)
    # Robert's branch is entered on the rows whose side disagrees with yhat: with left up to 6
    assert np.sum((np.where(pos, -yhat, yhat) > 0)) == 10 * ROWS_EACH
    want = np.array([float(x) for x in lines[n:]])
    z = np.array([kr.device_normal(seed, st, np.array([j], dtype=np.uint64))[0] for st, j in normals])
    assert ulps(z, want).max() <= 4, (z, want)
    assert len(set(want.tolist())) == len(want)


def test_restatement_flags_nonfinite_and_capped_rows():
    """A NaN or +-inf yhat takes no attempt and gives NaN; with the cap at 0 every finite row takes
    the truncated expectation (the arithmetic of both is tests/test_class_cpu.py's)."""
    yhat = np.array([np.nan, np.inf, -np.inf, 0.5, -3.0])
    pos = np.array([True, False, True, False, True])
    s, attempts, flag, _ = kr.class_sample_target(yhat, pos, 1, kr.CLASS_STREAM, np.arange(5))
    assert flag.tolist() == [1, 1, 1, 0, 0] and attempts[:3].tolist() == [0, 0, 0] and np.all(np.isnan(s[:3]))
    s, attempts, flag, _ = kr.class_sample_target(yhat[3:], pos[3:], 1, kr.CLASS_STREAM, np.arange(2), cap=0)
    assert flag.tolist() == [2, 2] and attempts.tolist() == [0, 0]
    assert s[0] == cr.expect_right(0.5) and s[1] == cr.expect_left(-3.0)


# ---- the oracle's task c against the compiled reference ------------------------------------------
@pytest.fixture(scope="module")
def cls_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("cls_oracle")


@pytest.mark.parametrize("name", ["cls_tiny/als_reg", "cls_tiny/mcmc", "cls_tiny_dup/mcmc", "cls_sa/als_reg",
                                  "cls_sa/mcmc"])
def test_oracle_task_c_vs_reference(name, cls_dir):
    """The reference's -task c runs through the oracle (the or_srand stream throughout): per iteration
    the correct counts exactly, alpha, ll_mcmc_this and the hyper-priors of the rlog to its six
    printed digits, then the -out predictions."""
    t = cr.load_trace(name)
    m = t["meta"]
    case = dc.Case(name, m["data"], m["dim"], m["seed"], m["iter"], init_stdev=m["init_stdev"], task="c",
                   method=m["method"], rng="reference", regular=m["regular"], threshold=m["threshold"])
    train, test = dc.oracle_data(dc.sources(case, cls_dir, None))
    assert (train.num_rows, test.num_rows) == (m["n_train"], m["n_test"])
    snaps, o = dc.oracle_chain(case, train, test)
    k = m["dim"][2]
    for it, (s, ref) in enumerate(zip(snaps, t["iters"])):
        r = ref["rlog"]
        assert s["n_train_correct"] == round(ref["train_acc"] * m["n_train"]), (it, s["n_train_correct"], ref)
        assert s["n_test_correct_all"] == round(ref["test_acc"] * m["n_test"]), (it, ref)
        assert s["n_test_correct_this"] == round(r["acc_mcmc_this"] * m["n_test"]), (it, ref)
        assert close(s["alpha"], r["alpha"]), (it, s["alpha"], r["alpha"])
        assert close(s["ll_this"], r["ll_mcmc_this"]), (it, s["ll_this"], r["ll_mcmc_this"])
        assert close(s["w_mu"][0], r["wmu[0]"]) and close(s["w_lambda"][0], r["wlambda[0]"]), (it, s["w_mu"], r)
        for f in range(k):
            assert close(s["v_mu"][f], r["vmu[0,%d]" % f]), (it, f)
            assert close(s["v_lambda"][f], r["vlambda[0,%d]" % f]), (it, f)
    pred, ref_pred = o.predict(), np.asarray(t["pred"])
    err = np.max(np.abs(pred - ref_pred) / np.abs(ref_pred))
    print("max relative difference of the predictions", err)
    assert err <= PRINT_REL


# ---- eligibility -----------------------------------------------------------------------------------
DEVICE_CASES = [c for c in dc.REGRESSION + dc.CLASSIFICATION if c.rng == "device"]


@pytest.mark.parametrize("case", DEVICE_CASES, ids=repr)
def test_chain_is_eligible(case, cls_dir, synth_files):
    """Two oracle chains from the restatement's start, the second with every normal moved to
    z + 4e-16 max(1, |z|) -- more than the device's log / cos / sqrt can differ from libm: they agree
    to 1e-11 in every iteration the GPU test runs (parameters, hyper-priors, alpha, w0, e, the
    iteration's RMSEs or correct counts). In task c every row's draw decides at a distance above 1e-9
    from its boundary in both chains, so the device cannot take another branch."""
    train, test = dc.oracle_data(dc.sources(case, cls_dir, synth_files))
    a, _ = dc.oracle_chain(case, train, test)
    b, _ = dc.oracle_chain(case, train, test, eps=dc.PERTURB)
    assert len(a) == len(b) == case.iters
    for it, (x, y) in enumerate(zip(a, b)):
        worst = dc.compare(case.task, y, x, {}, dc.ELIGIBLE)   # asserts each quantity finite and within the bound
        print(case, it, {k: "%.1e" % v for k, v in worst.items()}, "dist", x.get("dist"))
        assert max(worst.values()) <= dc.ELIGIBLE, (case, it, worst)
        if case.task == "c":
            assert min(x["dist"], y["dist"]) > dc.MIN_DIST, (case, it, x["dist"], y["dist"])
    assert not np.array_equal(a[0]["w"], b[0]["w"])        # (the second chain did take other normals)
    assert case.name not in dc.DROPPED


def test_every_layout_keeps_an_eligible_case():
    kept = [c for c in dc.REGRESSION if c.name not in dc.DROPPED]
    names = {c.name for c in kept}
    assert {"tiny/mcmc", "tiny/mcmc_meta"} & names            # entry store
    assert "tiny_dup/mcmc" in names                           # column layout, a repeated id
    assert any("level" in c.layouts and "column" in c.layouts for c in kept)


def test_keyed_normals_replace_only_the_attribute_draws(cls_dir):
    """With a source attached alpha, w0 and the hyper-priors still come from the or_srand stream:
    the first iteration's alpha and w0, drawn before any attribute, equal those of a chain without
    a source from the same start and seed; the attributes differ."""
    case = dc.by_name("tiny/mcmc")
    train, test = dc.oracle_data(dc.sources(case, cls_dir, None))
    D = oc.num_all_attribute(train, test)
    start = dc.start_params(case, D, 1)
    keyed, _ = dc.oracle_chain(case, train, test, start=start, iters=1)
    o = oc.ALS(*case.dim, D, None, method="mcmc")
    o.seed(case.seed)
    o.set_params(start)
    o.attach(train, test)
    o.iterate()
    assert o.s.alpha == keyed[0]["alpha"] and o.s.w0 == keyed[0]["w0"]
    assert not np.array_equal(o.params()["w"], keyed[0]["w"])


# ---- stream ids ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,iters", [(3, 6), (8, 10), (2, 8), (100, 25)])
def test_stream_ids_are_pairwise_distinct(k, iters):
    """Initialisation of v and w, the attribute sweeps per (iteration, factor) and the class rows per
    iteration: no two share a stream id of the seed. (With the initialisation on streams 21 and 22
    this failed: k = 3 reaches them in iteration 5, k = 8 in iteration 2, k = 2 in iteration 7.)"""
    table = kr.stream_table(k, iters)
    assert len(table) == 2 + iters * (k + 2)
    seen = {}
    for name, sid in table:
        assert 0 <= sid < 2 ** 64
        assert sid not in seen, "%s and %s share stream %d" % (seen[sid], name, sid)
        seen[sid] = name
    sweeps = [sid for name, sid in table if "sweep" in name]
    assert max(sweeps) < kr.INIT_STREAM and sorted(sweeps) == list(range(iters * (k + 1)))


@needs_gxx
def test_stream_table_is_the_librarys(check_exe):   # noqa: F811
    """The reserved ids of the table are the constants the library compiles in
    (csrc/vbfm_class_math.h: CLASS_STREAM, and INIT_STREAM_V / INIT_STREAM_W, which vbfm_mcmc_init
    passes to the initialisation), printed by class_math_check: if the library's ids moved back to
    21 and 22, this fails without a GPU."""
    r = subprocess.run([check_exe, "streams"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [int(x) for x in r.stdout.split()] == [kr.CLASS_STREAM, kr.INIT_V, kr.INIT_W]
    table = dict(kr.stream_table(3, 1))
    assert (table["init v"], table["init w"], table["iter 0 rows"]) == (kr.INIT_V, kr.INIT_W, kr.CLASS_STREAM)


# ---- the comparison itself -------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("side", ["got", "want"])
@pytest.mark.parametrize("key", ["w", "e", "alpha", "rmse_all"])
def test_compare_refuses_non_finite_values(key, side, bad):
    """A NaN or inf on either side of any quantity fails dc.compare (a plain max() fold would keep
    0.0 and pass); so does a difference above the bound, and equal snapshots pass."""
    def snap():
        s = {k: np.linspace(1.0, 2.0, 5) for k in dc.ARRAYS}
        s.update({k: 1.5 for k in dc.SCALARS["r"]})
        return s
    got, want = snap(), snap()
    assert max(dc.compare("r", got, want, {}, 1e-9).values()) == 0.0
    target = got if side == "got" else want
    if isinstance(target[key], np.ndarray):
        target[key][2] = bad
    else:
        target[key] = bad
    with pytest.raises(AssertionError):
        dc.compare("r", got, want, {}, 1e-9)
    off = snap()
    off["v"][0] += 1e-6
    with pytest.raises(AssertionError):
        dc.compare("r", off, snap(), {}, 1e-9)
    with pytest.raises(AssertionError):
        dc.rel_err(np.array([1.0, np.nan]), np.array([1.0, 1.0]))

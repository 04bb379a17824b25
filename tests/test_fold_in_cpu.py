"""Fold-in (include/vbfm.h "fold-in") without a GPU: the NumPy restatement of tests/fold_in_ref.py
against the exact fixed point of the sweep, its cheap invariances, the restated width table against
the source, bin/libFM's -fold_in flags through the stub launcher (host/libfm_main.cpp linked with
tests/cli_stub.cpp, which has none of the device entry points: the refusals are decided before any of
them is needed) and the host-only planner (csrc/vbfm_fold_plan.h) as a stand-alone program under
ASan + UBSan."""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fold_in_cases as fc
import fold_in_ref as ref
from conftest import ROOT, TESTS

PKG = os.path.join(ROOT, "scalable-variational-bayesian-factorization-machine_amd")
TINY = os.path.join(TESTS, "golden", "tiny")
TRAIN, TEST = os.path.join(TINY, "train.libfm"), os.path.join(TINY, "test.libfm")

# (k, k1, column lengths): short and long columns, with and without the linear term
FIXED_POINT_CASES = [(1, 1, (3, 40)), (3, 0, (5, 17)), (8, 1, (2, 9, 200)), (20, 1, (30, 300))]
FIXED_POINT_IDS = ["k%d-k1_%d" % (k, k1) for k, k1, _ in FIXED_POINT_CASES]
FIXED_POINT_BOUND = 1e-12
MOST_PASSES = 2000


def fixed_point_data(case):
    k, k1, lengths = case
    _, model = fc.model(k, 1, k1, seed=5)
    rows, y, _, _ = fc.interleave(fc.columns(lengths, 300 + k), 7)
    return model, rows, y


def distance(got_w, got_v, want_w, want_v):
    """The largest difference of the means, relative to the largest mean of the solve (at least 1)."""
    scale = max(1.0, float(np.max(np.abs(want_w))), float(np.max(np.abs(want_v))) if want_v.size else 0.0)
    d = float(np.max(np.abs(got_w - want_w)))
    return max(d, float(np.max(np.abs(got_v - want_v))) if want_v.size else 0.0) / scale


@functools.lru_cache(maxsize=None)
def fixed_point(case):
    """(T, distance): the first pass count at which the restatement's means of every column are within
    FIXED_POINT_BOUND of the solve, and the distance there. Measured on the CPU; tests/test_fold_in_gpu.py
    runs the device for T passes and never takes T from it."""
    model, rows, y = fixed_point_data(case)
    want = ref.fold_in(model, rows, y, passes=1, solve=True)
    lo, T = 0, 16
    while True:                                   # the distance shrinks with the passes: bracket, then bisect
        got = ref.fold_in(model, rows, y, passes=T)
        if distance(got["mu_w"], got["mu_v"], want["mu_w"], want["mu_v"]) <= FIXED_POINT_BOUND:
            break
        assert T < MOST_PASSES, "the sweep does not reach the solve"
        lo, T = T, 2 * T
    while T - lo > 1:
        mid = (lo + T) // 2
        got = ref.fold_in(model, rows, y, passes=mid)
        if distance(got["mu_w"], got["mu_v"], want["mu_w"], want["mu_v"]) <= FIXED_POINT_BOUND:
            T = mid
        else:
            lo = mid
    got = ref.fold_in(model, rows, y, passes=T)
    return T, distance(got["mu_w"], got["mu_v"], want["mu_w"], want["mu_v"])


@pytest.mark.parametrize("case", FIXED_POINT_CASES, ids=FIXED_POINT_IDS)
def test_the_sweep_reaches_the_solve(case):
    """The sweep is Gauss-Seidel on (diag(lambda) + alpha sum x^2 B + alpha Phi'Phi) m = alpha Phi'(y - base):
    the restatement is within 1e-12 of numpy.linalg.solve after T passes, and stays there."""
    T, d = fixed_point(case)
    print("k=%d k1=%d lengths=%s: T=%d distance %.3e" % (case[0], case[1], case[2], T, d))
    assert 1 <= T <= MOST_PASSES and d <= FIXED_POINT_BOUND
    model, rows, y = fixed_point_data(case)
    want = ref.fold_in(model, rows, y, passes=1, solve=True)
    got = ref.fold_in(model, rows, y, passes=2 * T)
    assert distance(got["mu_w"], got["mu_v"], want["mu_w"], want["mu_v"]) <= FIXED_POINT_BOUND
    # e after the sweep is the target minus the extended model's unclipped mean
    mean = ref.score(ref.extended(model, got), rows)
    assert np.max(np.abs(got["resid"] - (y.astype(np.float64) - mean))) <= 1e-12 * max(1.0, np.max(np.abs(mean)))


def test_a_column_does_not_depend_on_the_others():
    _, model = fc.model(3, 1, 1)
    cols = fc.columns((5, 0, 9, 2), 11)
    rows, y, col_of_row, _ = fc.interleave(cols, 3)
    whole = ref.fold_in(model, rows, y, passes=6)
    for c in (0, 2, 3):
        alone_cols = [r if i == c else [] for i, r in enumerate(cols)]
        r1, y1, _, _ = fc.interleave(alone_cols, 5)
        alone = ref.fold_in(model, r1, y1, passes=6, num_attribute=fc.D + len(cols))
        for key in ("mu_w", "sigma_w"):
            assert alone[key][c] == whole[key][c]
        for key in ("mu_v", "sigma_v"):
            assert np.array_equal(alone[key][:, c], whole[key][:, c])
        assert np.array_equal(alone["resid"], whole["resid"][col_of_row == c])
    assert whole["sigma_w"][1] == 1.0 / whole["prior_used"][0] and whole["mu_w"][1] == 0.0   # an id without rows
    assert np.array_equal(whole["sigma_v"][:, 1], 1.0 / whole["prior_used"][1:])


def test_shuffling_rows_across_columns_keeps_the_bits():
    _, model = fc.model(8, 0, 1)
    cols = fc.columns((4, 7, 1, 12), 21)
    a_rows, a_y, a_col, a_idx = fc.interleave(cols, 1)
    b_rows, b_y, b_col, b_idx = fc.interleave(cols, 2)
    assert not np.array_equal(a_col, b_col)
    a, b = ref.fold_in(model, a_rows, a_y, passes=5, tol=1e-3), ref.fold_in(model, b_rows, b_y, passes=5, tol=1e-3)
    for key in ("mu_w", "sigma_w", "mu_v", "sigma_v", "col_passes"):
        assert np.array_equal(a[key], b[key])
    key_a, key_b = np.lexsort((a_idx, a_col)), np.lexsort((b_idx, b_col))
    assert np.array_equal(a["resid"][key_a], b["resid"][key_b])


def test_guards_keep_the_old_mean():
    """An infinite target: every mean of that column stays 0, the sigmas stay finite, every update is
    counted; the neighbours are what they are without it."""
    _, model = fc.model(3, 1, 1)
    cols = fc.columns((4, 5, 3), 31)
    rows, y, col_of_row, idx = fc.interleave(cols, 4)
    clean = ref.fold_in(model, rows, y, passes=4)
    y2 = y.copy()
    y2[np.nonzero(col_of_row == 1)[0][2]] = np.inf
    bad = ref.fold_in(model, rows, y2, passes=4)
    assert bad["mu_w"][1] == 0.0 and np.all(bad["mu_v"][:, 1] == 0.0)
    assert np.isfinite(bad["sigma_w"][1]) and np.all(np.isfinite(bad["sigma_v"][:, 1]))
    assert bad["stats"]["nonfinite_updates"] == 4 * (1 + 3) and clean["stats"]["nonfinite_updates"] == 0
    for c in (0, 2):
        assert bad["mu_w"][c] == clean["mu_w"][c] and np.array_equal(bad["mu_v"][:, c], clean["mu_v"][:, c])


def test_the_heldout_set_clears_its_test_on_the_cpu():
    """The set of tests/test_fold_in_gpu.py::test_fold_in_beats_skipping, chosen here: with the oracle's
    parameters the restatement's RMSE on the held-out users' other rows is well below that of scoring
    them with the new id skipped (0.659 against 0.970)."""
    D, block, train, (s_rows, s_y), (t_rows, t_y) = fc.heldout_set()
    _, model = fc.heldout_model(D, train)
    folded = ref.fold_in(model, s_rows, s_y, passes=20, prior_ids=block)
    with_fold = np.clip(ref.score(ref.extended(model, folded), t_rows), 1.0, 5.0)
    skipped = np.clip(ref.frozen_sums(model, ref.split_rows(D, *t_rows)[2])[0], 1.0, 5.0)
    rmse = [float(np.sqrt(np.mean((p - t_y) ** 2))) for p in (with_fold, skipped)]
    print("RMSE with fold-in %.4f, with the new id skipped %.4f" % tuple(rmse))
    assert rmse[0] < 0.8 * rmse[1]


# ---- the width table ---------------------------------------------------------------------------------
def test_restated_table_is_the_library_s():
    with open(os.path.join(PKG, "csrc", "vbfm_fold_plan.h")) as fh:
        src = fh.read()
    assert int(re.search(r"constexpr int FOLD_R = (\d+);", src).group(1)) == fc.FOLD_R
    assert int(re.search(r"constexpr int FOLD_WG = (\d+);", src).group(1)) == fc.FOLD_WG
    assert int(re.search(r"constexpr uint32_t FOLD_WG_LDS_ROWS = (\d+);", src).group(1)) == fc.FOLD_WG_LDS_ROWS
    body = src[src.index("inline int fold_auto_width("):]
    body = body[:body.index("\n}")]
    lo, hi = (int(v) for v in re.search(r"for \(int g = (\d+); g <= (\d+); g \*= 2\)", body).groups())
    factor = int(float(re.search(r"if \(mean <= ([\d.]+) \* g\) return g;", body).group(1)))
    table = [(factor * g, g) for g in (4, 8, 16, 32, 64) if lo <= g <= hi]
    last = re.search(r"return mean <= ([\d.]+) \* FOLD_R \? (\d+) : FOLD_WG;", body)
    table.append((int(float(last.group(1))) * fc.FOLD_R, int(last.group(2))))
    assert tuple(table) == fc.AUTO_TABLE
    widths = re.search(r"inline bool fold_width_ok\(int g\) \{ return (.*); \}", src).group(1)
    assert tuple(int(g) if g.isdigit() else fc.FOLD_WG for g in re.findall(r"g == (\w+)", widths)) == fc.WIDTHS


@pytest.mark.parametrize("G", fc.WIDTHS)
def test_every_case_lands_in_its_width_and_path(G):
    lengths = fc.column_lengths(G)
    assert len(set(lengths)) == len(lengths) and lengths == sorted(lengths), "width %d: the lengths collide" % G
    got = [fc.path(G, n) for n in lengths]
    assert got == fc.EXPECTED_PATHS[G], "width %d: columns of %s rows take %s" % (G, lengths, got)
    # either side of every threshold is there
    gr = fc.group_rows(G)
    assert gr in lengths and gr + 1 in lengths and fc.path(G, gr) != fc.path(G, gr + 1)


def test_auto_width_bands():
    for upper, g in fc.AUTO_TABLE:
        assert fc.auto_width(upper * 10, 10) == g
        assert fc.auto_width(upper * 10 + 1, 10) != g
    assert fc.auto_width(0, 0) == 4 and fc.auto_width(10 ** 6, 1) == fc.FOLD_WG


# ---- the launcher's flags ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stub_cli(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stub_fold") / "libfm_stub")
    subprocess.run(["g++", "-std=c++17", "-O0", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(PKG, "host", "libfm_main.cpp"), os.path.join(PKG, "csrc", "vbfm_host.cpp"),
                    os.path.join(TESTS, "cli_stub.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    return exe


def run(exe, args, cwd):
    return subprocess.run([exe] + args, cwd=str(cwd), capture_output=True, text=True, timeout=120)


FOLD = ["-fold_in", TRAIN]


@pytest.mark.parametrize("args,message", [
    (["-test", TEST, "-out", "p", "-fold_passes", "3"], "-fold_passes needs -fold_in"),
    (["-test", TEST, "-out", "p", "-fold_tol", "1e-6"], "-fold_tol needs -fold_in"),
    (["-test", TEST, "-out", "p", "-fold_prior_ids", "0,4"], "-fold_prior_ids needs -fold_in"),
    (["-test", TEST, "-out", "p", "-fold_prior", "1,2"], "-fold_prior needs -fold_in"),
    (["-test", TEST, "-out", "p", "-save_model", "m2"], "-save_model with -load_model writes the model -fold_in extends"),
    (FOLD, "-fold_in needs -save_model or -test"),
    (FOLD + ["-save_model", "m2", "-out", "p"], "-out needs -test"),
    (FOLD + ["-test", TEST], "-load_model needs -test and -out"),
    (FOLD + ["-test", TEST, "-out", "p", "-fold_passes", "0"], "-fold_passes needs a whole number >= 1, not '0'"),
    (FOLD + ["-test", TEST, "-out", "p", "-fold_passes", "3x"], "-fold_passes needs a whole number >= 1, not '3x'"),
    (FOLD + ["-test", TEST, "-out", "p", "-fold_passes", "2.5"], "-fold_passes needs a whole number >= 1"),
    (FOLD + ["-test", TEST, "-out", "p", "-fold_tol", "nan"], "-fold_tol needs a finite number >= 0, not 'nan'"),
    (FOLD + ["-test", TEST, "-out", "p", "-fold_tol", "-1e-3"], "-fold_tol needs a finite number >= 0"),
    (FOLD + ["-test", TEST, "-out", "p", "-fold_tol", "1e-3q"], "-fold_tol needs a finite number >= 0"),
    (FOLD + ["-test", TEST, "-out", "p", "-fold_prior_ids", "4"], "-fold_prior_ids needs LO,HI"),
    (FOLD + ["-test", TEST, "-out", "p", "-fold_prior_ids", "4,4"], "-fold_prior_ids needs LO,HI"),
    (FOLD + ["-test", TEST, "-out", "p", "-fold_prior_ids", "a,4"], "-fold_prior_ids needs LO,HI"),
    (FOLD + ["-test", TEST, "-out", "p", "-fold_prior", "1"], "-fold_prior needs W,V"),
    (FOLD + ["-test", TEST, "-out", "p", "-fold_prior", "1,0"], "-fold_prior needs W,V"),
    (FOLD + ["-test", TEST, "-out", "p", "-fold_prior", "inf,1"], "-fold_prior needs W,V"),
    (FOLD + ["-test", TEST, "-out", "p", "-fold_prior", "1,x"], "-fold_prior needs W,V"),
    # well-formed: the build is then what is missing (the stub has no fold-in entry point)
    (FOLD + ["-test", TEST, "-out", "p", "-fold_passes", "5", "-fold_tol", "1e-6", "-fold_prior_ids", "0,4", "-fold_prior", "1,2.5",
             "-save_model", "m2"], "this build has no fold-in"),
    (FOLD + ["-save_model", "m2"], "this build has no fold-in"),
    (FOLD + ["-test", TEST, "-candidates", TRAIN, "-topn", "3", "-ucb", "1.5", "-out", "p"], "this build has no fold-in"),
])
def test_flag_refusals_inside_load_model(stub_cli, tmp_path, args, message):
    r = run(stub_cli, ["-load_model", "m"] + args, tmp_path)
    assert "ERROR: " + message in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(tmp_path / "p") and not os.path.exists(tmp_path / "m2")


@pytest.mark.parametrize("extra", [FOLD, ["-fold_passes", "3"], ["-fold_tol", "1e-6"], ["-fold_prior_ids", "0,4"],
                                   ["-fold_prior", "1,2"]])
def test_the_flags_are_refused_outside_load_model(stub_cli, tmp_path, extra):
    r = run(stub_cli, ["-task", "r", "-train", TRAIN, "-test", TEST, "-method", "vb", "-dim", "1,1,2", "-iter", "1",
                       "-seed", "3"] + extra, tmp_path)
    assert "ERROR: -fold_in and its -fold_* flags belong to -load_model" in r.stderr, r.stderr[-2000:]


def test_help_lists_the_flags(stub_cli, tmp_path):
    r = run(stub_cli, ["-help"], tmp_path)
    for flag in ("-fold_in", "-fold_passes", "-fold_tol", "-fold_prior_ids", "-fold_prior"):
        assert flag in r.stdout + r.stderr


# ---- the planner ---------------------------------------------------------------------------------------
@pytest.mark.skipif(not shutil.which("g++"), reason="needs g++")
def test_planner_under_asan_ubsan(tmp_path):
    """tests/fold_plan_check.cpp (its own main) over csrc/vbfm_fold_plan.h, which takes no HIP type and
    compiles on its own, under ASan + UBSan. Nothing is loaded into Python under a sanitizer."""
    from test_host_sanitizers import SAN
    exe = str(tmp_path / "fold_plan_check")
    subprocess.run(["g++", "-std=c++17", *SAN, "-Wall", "-Werror", "-static-libasan", "-static-libubsan", "-pthread",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(TESTS, "fold_plan_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-8000:]
    assert "fold plan check ok" in r.stdout

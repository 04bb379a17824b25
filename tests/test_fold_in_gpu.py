"""vbfm_fold_in on the GPU (include/vbfm.h "fold-in") against the NumPy restatement of
tests/fold_in_ref.py: every lane width and path (tests/fold_in_cases.py), the frozen part, bit-identity
across chunk sizes and row orders, the residuals, the fixed point, tol, the guards, the consumers of
the extended model, vbfm_model_write and the refusals. Models are written from synthetic parameters
with Model.write_params; nothing trains.

Tolerance: REL = 1e-9 by rel_err, the project's bound for a reordered fp64 sum (tests/test_score_gpu.py):
the device adds a column's rows across lanes, the restatement in row order."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import fold_in_cases as fc
import fold_in_ref as ref
import vbfm
from test_fold_in_cpu import FIXED_POINT_CASES, FIXED_POINT_IDS, fixed_point, fixed_point_data
from test_score_gpu import assert_bits, rel_err

pytestmark = pytest.mark.gpu
REL = 1e-9
COUNTS = ("new_attributes", "with_rows", "longest_column", "passes_max", "not_converged", "rows", "nonfinite_updates")


@functools.lru_cache(maxsize=None)
def support(G):
    """The support rows of width G's case (they do not depend on k): rows, target, column of every
    row, its index in the column, and the restatement's split of the rows."""
    cols = fc.columns(fc.column_lengths(G), 40 + G)
    rows, y, col_of_row, idx = fc.interleave(cols, G)
    return cols, rows, y, col_of_row, idx, ref.split_rows(fc.D, *rows)


def load(tmp_path, info, p, name="m", task="r"):
    path = str(tmp_path / name)
    vbfm.Model.write_params(path, info, p, task=task)
    return vbfm.Model.load(path), path


def new_params(m, tmp_path, D, name="ext"):
    """The new ids' parameters of an extended model, through Model.save + Model.read_params."""
    path = str(tmp_path / name)
    m.save(path)
    p = vbfm.Model.read_params(path)
    k, D_out = p["info"]["num_factor"], p["info"]["num_attribute"]
    return dict(mu_w=p["mu_w"][D:], sigma_w=p["sigma_w"][D:], mu_v=p["mu_v"].reshape(k, D_out)[:, D:],
                sigma_v=p["sigma_v"].reshape(k, D_out)[:, D:]), path


def check(got, resid, st, want, what):
    for key in ("mu_w", "sigma_w", "mu_v", "sigma_v"):
        err = rel_err(got[key], want[key])
        print("%s %s: rel err %.3e" % (what, key, err))
        assert err <= REL, (what, key, err)
    err = rel_err(resid, want["resid"])
    print("%s resid: rel err %.3e" % (what, err))
    assert err <= REL, (what, "resid", err)
    assert rel_err(st["prior_used"], want["prior_used"]) <= 1e-12, (what, st["prior_used"], want["prior_used"])
    for key in COUNTS:
        assert st[key] == want["stats"][key], (what, key, st[key], want["stats"][key])


# ---- 1. every width and path ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", fc.KS)
@pytest.mark.parametrize("G", fc.WIDTHS)
def test_every_width_and_path_against_the_restatement(tmp_path, G, k):
    _, rows, y, _, _, split = support(G)
    for k1, k0, pri in fc.variants(G, k):
        info, p = fc.model(k, k0, k1)
        m, _ = load(tmp_path, info, p)
        ext, st, resid = m.fold_in(rows + (y,), passes=3, lanes=G, residuals=True, **pri)
        want = ref.fold_in(p, rows, y, passes=3, split=split, **pri)
        got, _ = new_params(ext, tmp_path, fc.D)
        assert st["lanes"] == G and ext.info["num_attribute"] == fc.D + len(fc.column_lengths(G))
        check(got, resid, st, want, "G=%d k=%d k1=%d k0=%d %s" % (G, k, k1, k0, "given" if "prior_w" in pri else "derived"))
        ext.close()
        m.close()


@pytest.mark.parametrize("mean_rows,G", [(3, 4), (12, 8), (30, 16), (60, 32), (200, 64), (300, fc.FOLD_WG)])
def test_auto_width(tmp_path, mean_rows, G):
    """lanes = 0 picks the width of the table from the mean rows per non-empty column, and the result is
    that width's, bit for bit."""
    assert fc.auto_width(mean_rows * 3, 3) == G
    info, p = fc.model(3, 1, 1)
    rows, y, _, _ = fc.interleave(fc.columns((mean_rows - 1, 0, mean_rows, mean_rows + 1), 3), 8)
    m, _ = load(tmp_path, info, p)
    a, st, ra = m.fold_in(rows + (y,), passes=2, residuals=True)
    b, _, rb = m.fold_in(rows + (y,), passes=2, lanes=G, residuals=True)
    assert st["lanes"] == G
    pa, fa = new_params(a, tmp_path, fc.D, "a")
    pb, fb = new_params(b, tmp_path, fc.D, "b")
    assert open(fa, "rb").read() == open(fb, "rb").read()
    assert_bits(ra, rb, "resid")


# ---- 2. the frozen part and the input handle -------------------------------------------------------------
def test_frozen_part_and_input_handle(tmp_path):
    G, k = 8, 8
    _, rows, y, _, _, _ = support(G)
    info, p = fc.model(k, 1, 1)
    m, path = load(tmp_path, info, p)
    probe = fc.interleave(fc.columns((6,), 5), 1)[0]
    probe = (probe[0], np.minimum(probe[1], fc.D - 1).astype(np.uint32), probe[2])   # ids the model has
    before = m.score(probe, variance=True, clip=False)
    ext, _ = m.fold_in(rows + (y,), passes=2)
    after = m.score(probe, variance=True, clip=False)
    assert_bits(before[0], after[0], "mean")
    assert_bits(before[1], after[1], "T")
    assert m.info["num_attribute"] == fc.D
    _, ext_path = new_params(ext, tmp_path, fc.D)
    old, new = open(path, "rb").read(), open(ext_path, "rb").read()
    D_out = ext.info["num_attribute"]
    # the payload after the 88-byte header: w pairs [D], then v pairs [j*k + f]
    assert new[88:88 + 16 * fc.D] == old[88:88 + 16 * fc.D]
    assert new[88 + 16 * D_out:88 + 16 * D_out + 16 * k * fc.D] == old[88 + 16 * fc.D:]
    for key in ("kind", "k0", "k1", "num_factor", "min_target", "max_target", "iter", "has_variance", "w0_or_mu0",
                "sigma_0_dash", "alpha"):
        assert ext.info[key] == m.info[key], key
    assert ext.task == m.task


# ---- 3. bit-identity ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [4, 32, fc.FOLD_WG])
def test_bit_identity_across_chunks_and_row_orders(tmp_path, G):
    k = 8
    cols, rows, y, col_of_row, idx, _ = support(G)
    info, p = fc.model(k, 1, 1)
    m, _ = load(tmp_path, info, p)
    key = np.lexsort((idx, col_of_row))
    want_file, want_resid = None, None
    runs = [(rows, y, key, cb) for cb in (1, 4096, 1 << 16, 0)]
    rows2, y2, col2, idx2 = fc.interleave(cols, 99)
    assert not np.array_equal(col2, col_of_row)
    runs.append((rows2, y2, np.lexsort((idx2, col2)), 0))
    chunks = []
    for i, (r, t, order, cb) in enumerate(runs):
        ext, st, resid = m.fold_in(r + (t,), passes=4, lanes=G, chunk_bytes=cb, residuals=True, tol=1e-4)
        chunks.append(st["n_chunks"])
        _, path = new_params(ext, tmp_path, fc.D, "ext%d" % i)
        data = open(path, "rb").read()
        if want_file is None:
            want_file, want_resid = data, resid[order]
        assert data == want_file, (G, cb, i)
        assert_bits(resid[order], want_resid, "resid of run %d" % i)
        ext.close()
    assert chunks[0] == len(cols) and chunks[3] == 1 and chunks[0] > chunks[1] >= chunks[2] >= 1, chunks


# ---- 4. the residuals ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,k", [(8, 3), (64, 65), (fc.FOLD_WG, 8)])
def test_residuals_are_the_extended_model_s(tmp_path, G, k):
    _, rows, y, _, _, _ = support(G)
    info, p = fc.model(k, 1, 1)
    m, _ = load(tmp_path, info, p)
    ext, _, resid = m.fold_in(rows + (y,), passes=5, lanes=G, residuals=True)
    mean = ext.score(rows, clip=False, order="group")
    want = y.astype(np.float64) - mean
    err = rel_err(resid, want)
    print("G=%d k=%d: resid against target - score: rel err %.3e" % (G, k, err))
    assert err <= REL


# ---- 5. the fixed point ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FIXED_POINT_CASES, ids=FIXED_POINT_IDS)
def test_fixed_point(tmp_path, case):
    """At the pass count T measured on the CPU (tests/test_fold_in_cpu.py) the device is within that
    test's distance + 1e-9 of numpy.linalg.solve."""
    T, d = fixed_point(case)
    model, rows, y = fixed_point_data(case)
    m, _ = load(tmp_path, model["info"], model)
    ext, st = m.fold_in(rows + (y,), passes=T)
    got, _ = new_params(ext, tmp_path, fc.D)
    want = ref.fold_in(model, rows, y, passes=1, solve=True)
    scale = max(1.0, float(np.max(np.abs(want["mu_w"]))), float(np.max(np.abs(want["mu_v"]))))
    dist = max(float(np.max(np.abs(got["mu_w"] - want["mu_w"]))), float(np.max(np.abs(got["mu_v"] - want["mu_v"])))) / scale
    print("k=%d: T=%d, CPU distance %.3e, device distance %.3e" % (case[0], T, d, dist))
    assert st["passes_max"] == T
    assert dist <= d + 1e-9


# ---- 6. tol -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes,tol", [(6, 1e-12), (300, 1e-6), (40, 1e-3)])
def test_tol_pass_counts(tmp_path, passes, tol):
    lengths = (1, 5, 0, 9, 40, 130)
    cols = fc.columns(lengths, 77)
    rows, y, _, _ = fc.interleave(cols, 6)
    info, p = fc.model(3, 1, 1)
    m, _ = load(tmp_path, info, p)
    want = ref.fold_in(p, rows, y, passes=passes, tol=tol)
    _, st = m.fold_in(rows + (y,), passes=passes, tol=tol, lanes=8)
    print("passes=%d tol=%g: per column %s, not converged %d" % (passes, tol, want["col_passes"], want["stats"]["not_converged"]))
    assert st["passes_max"] == want["stats"]["passes_max"] and st["not_converged"] == want["stats"]["not_converged"]
    # a column's pass count: the call that holds that column alone (columns do not interact)
    for c, n in enumerate(lengths):
        alone = fc.interleave([r if i == c else [] for i, r in enumerate(cols)], 1)
        _, st1 = m.fold_in(alone[0] + (alone[1],), passes=passes, tol=tol, lanes=8, num_attribute=fc.D + len(cols))
        want1 = ref.fold_in(p, alone[0], alone[1], passes=passes, tol=tol, num_attribute=fc.D + len(cols))
        assert want1["col_passes"][c] == want["col_passes"][c], (c, n)
        assert st1["passes_max"] == want["col_passes"][c], (c, n)
        assert st1["not_converged"] == want1["stats"]["not_converged"], (c, n)


# ---- 7. the guards -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [4, fc.FOLD_WG])
def test_guards(tmp_path, G):
    k = 3
    cols = fc.columns((4, 5, 3, 40), 31)
    rows, y, col_of_row, _ = fc.interleave(cols, 4)
    y = y.copy()
    y[np.nonzero(col_of_row == 1)[0][2]] = np.inf
    info, p = fc.model(k, 1, 1)
    m, _ = load(tmp_path, info, p)
    ext, st, resid = m.fold_in(rows + (y,), passes=4, lanes=G, residuals=True)
    want = ref.fold_in(p, rows, y, passes=4)
    got, _ = new_params(ext, tmp_path, fc.D)
    assert got["mu_w"][1] == 0.0 and np.all(got["mu_v"][:, 1] == 0.0)
    assert np.isfinite(got["sigma_w"][1]) and np.all(np.isfinite(got["sigma_v"][:, 1]))
    assert st["nonfinite_updates"] == want["stats"]["nonfinite_updates"] == 4 * (1 + k)
    for key in ("mu_w", "sigma_w", "mu_v", "sigma_v"):     # the neighbours, and the column's own sigmas
        assert rel_err(got[key], want[key]) <= REL, key
    finite = np.isfinite(y)
    assert rel_err(resid[finite], want["resid"][finite]) <= REL
    assert np.isinf(resid[~finite]).all() and (~finite).sum() == 1


# ---- 8. the consumers ----------------------------------------------------------------------------------------------
def test_consumers_take_the_extended_model(tmp_path):
    G, k = 8, 8
    cols, rows, y, _, _, _ = support(G)
    info, p = fc.model(k, 1, 1)
    m, _ = load(tmp_path, info, p)
    ext, _ = m.fold_in(rows + (y,), passes=5)
    _, path = new_params(ext, tmp_path, fc.D)
    again = vbfm.Model.load(path)
    contexts = (rows[0][:41], rows[1][:int(rows[0][40])], rows[2][:int(rows[0][40])])   # 40 support rows: new ids inside
    items = fc.interleave(fc.columns((25,), 9), 1)[0]
    items = (items[0], np.minimum(items[1], fc.D - 1).astype(np.uint32), items[2])
    res = []
    for mod in (ext, again):
        out = list(mod.score(contexts, variance=True))
        cs = mod.candidates(items, variance=True)
        out += list(mod.recommend(contexts, cs, 5))
        out += list(mod.recommend_ucb(contexts, cs, 5, 1.5, noise=True))
        cs.close()
        res.append(out)
    for a, b in zip(*res):
        assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
    first_new = int(min(j for j in contexts[1][:int(contexts[0][1])] if j >= fc.D))
    cs = m.candidates(items, variance=True)
    for call in (lambda: m.score(contexts, variance=True), lambda: m.recommend(contexts, cs, 5),
                 lambda: m.recommend_ucb(contexts, cs, 5, 1.5)):
        with pytest.raises(vbfm.VbfmError, match="row 0 holds feature id %d" % first_new):
            call()
    cs.close()


# ---- 9. vbfm_model_write ---------------------------------------------------------------------------------------------
def test_model_write_reproduces_files(tmp_path):
    info, p = fc.model(3, 1, 1)
    als = dict(info, kind=2, has_variance=0, sigma_0_dash=0.0)
    files = []
    vbfm.Model.write_params(str(tmp_path / "vb"), info, p)
    vbfm.Model.write_params(str(tmp_path / "als"), als, dict(w=p["mu_w"], v=p["mu_v"]))
    vbfm.Model.write_params(str(tmp_path / "cls"), dict(als, kind=3), dict(w=p["mu_w"], v=p["mu_v"]), task="c")
    for name in ("vb", "als", "cls"):
        m = vbfm.Model.load(str(tmp_path / name))
        m.save(str(tmp_path / (name + "2")))
        assert open(tmp_path / name, "rb").read() == open(tmp_path / (name + "2"), "rb").read(), name
        files.append(name)
        m.save(str(tmp_path / (name + "3")), num_iter=99)
        assert vbfm.Model.file_info(str(tmp_path / (name + "3")))["iter"] == 99
    draws = [dict(w=p["mu_w"], v=p["mu_v"], w0=0.1, alpha=1.0), dict(w=p["sigma_w"], v=p["sigma_v"], w0=0.2, alpha=2.0)]
    vbfm.Model.write_chain(str(tmp_path / "chain"), dict(als, kind=4), draws)
    ch = vbfm.Model.load(str(tmp_path / "chain"))
    with pytest.raises(vbfm.VbfmError, match="vbfm_chain_save"):
        ch.save(str(tmp_path / "chain2"))
    assert not os.path.exists(tmp_path / "chain2")


# ---- 10. the refusals ------------------------------------------------------------------------------------------------
def test_refusals(tmp_path):
    L = vbfm.lib()
    info, p = fc.model(3, 1, 1)
    m, _ = load(tmp_path, info, p)
    rows, y, _, _ = fc.interleave(fc.columns((4, 2), 3), 1)
    probe = (rows[0], np.minimum(rows[1], fc.D - 1).astype(np.uint32), rows[2])
    before = m.score(probe, clip=False)
    data = rows + (y,)

    def refused(model, word, **kw):
        with pytest.raises(vbfm.VbfmError, match=word):
            model.fold_in(kw.pop("data", data), **kw)

    refused(m, "passes = 0", passes=0)
    refused(m, "prior_w = -1", prior_w=-1.0)
    refused(m, "prior_w = inf", prior_w=np.inf)
    refused(m, r"prior_v\[1\] = 0", prior_v=[1.0, 0.0, 1.0])
    refused(m, r"prior_v\[2\] = -?nan", prior_v=[1.0, 1.0, np.nan])
    refused(m, r"prior id range \[5, 5\)", prior_ids=(5, 5))
    refused(m, r"prior id range \[7, 3\)", prior_ids=(7, 3))
    refused(m, r"prior id range \[0, 41\)", prior_ids=(0, fc.D + 1))
    refused(m, "lanes = 128", lanes=128)
    none = (np.array([0, 2, 4], dtype=np.uint64), np.array([1, 41, 2, 3], dtype=np.uint32), np.ones(4, dtype=np.float32),
            np.ones(2, dtype=np.float32))
    refused(m, "row 1 holds no new feature id", data=none)
    refused(m, "but num_attribute_out = 41", num_attribute=fc.D + 1)
    two = (np.array([0, 3], dtype=np.uint64), np.array([1, 44, 47], dtype=np.uint32), np.ones(3, dtype=np.float32), np.ones(1, dtype=np.float32))
    refused(m, r"row 0 holds two new feature ids \(44 and 47\)", data=two)
    # a derived prior that is not finite: nothing to derive it from
    zero = dict(p, mu_w=np.zeros(fc.D), sigma_w=np.zeros(fc.D))
    mz, _ = load(tmp_path, info, zero, "zero")
    refused(mz, "prior derived over the ids .* for w is inf")
    # a kind without a posterior
    als = dict(info, kind=2, has_variance=0, sigma_0_dash=0.0)
    ma, _ = load(tmp_path, als, dict(w=p["mu_w"], v=p["mu_v"]), "als")
    refused(ma, "a model of kind VBFM_MODEL_ALS")
    # more factors than the kernels take
    wide, pw = fc.model(257, 1, 1, d=4)
    mw, _ = load(tmp_path, wide, pw, "wide")
    refused(mw, "num_factor = 257", data=(np.array([0, 1], dtype=np.uint64), np.array([5], dtype=np.uint32), np.ones(1, dtype=np.float32),
                                          np.ones(1, dtype=np.float32)))
    # null arguments through the C call: *out stays NULL
    csr, keep = m._rows(rows)
    o = vbfm.FoldOpts(3, 0.0, 0.0, None, 0, 0, 0, 0, 0)
    yp = y.ctypes.data_as(C.POINTER(C.c_float))
    for args, word in (((m._m, None, yp, C.byref(o)), "null rows"), ((m._m, C.byref(csr), None, C.byref(o)), "null target"),
                       ((m._m, C.byref(csr), yp, None), "null options")):
        h = C.c_void_p(1)
        assert L.vbfm_fold_in(C.byref(h), *args, None, None, None) != 0
        assert h.value is None and word in L.vbfm_model_last_error(m._m).decode()
    assert L.vbfm_fold_in(None, m._m, C.byref(csr), yp, C.byref(o), None, None, None) != 0
    assert "null out" in L.vbfm_model_last_error(m._m).decode()
    h = C.c_void_p(1)
    assert L.vbfm_fold_in(C.byref(h), None, C.byref(csr), yp, C.byref(o), None, None, None) != 0 and h.value is None
    o.passes = 0
    h = C.c_void_p(1)
    assert L.vbfm_fold_in(C.byref(h), m._m, C.byref(csr), yp, C.byref(o), None, None, None) != 0 and h.value is None
    # after every refusal the model scores as before, and folds in
    assert_bits(m.score(probe, clip=False), before, "scores after the refusals")
    ext, st = m.fold_in(data, passes=2)
    assert st["new_attributes"] == 2 and ext.info["num_attribute"] == fc.D + 2


# ---- 11. the point of it -----------------------------------------------------------------------------------------------
def test_fold_in_beats_skipping(tmp_path):
    """Users the model has never seen (tests/fold_in_cases.py heldout_set: a planted-model set, the VB
    parameters from the C oracle), folded in from half of their rows and scored on the other half:
    RMSE 0.659 with fold-in against 0.970 with unknown_ids="skip" (the restatement's figures, chosen
    on the CPU by tests/test_fold_in_cpu.py; the device's are printed)."""
    D, block, train, (s_rows, s_y), (t_rows, t_y) = fc.heldout_set()
    info, p = fc.heldout_model(D, train)
    m, _ = load(tmp_path, info, p)
    ext, st = m.fold_in(s_rows + (s_y,), passes=20, prior_ids=block)
    assert st["new_attributes"] == fc.HELD_USERS and st["with_rows"] == fc.HELD_USERS
    with_fold = ext.score(t_rows)
    skipped = m.score(t_rows, unknown_ids="skip")
    rmse = [float(np.sqrt(np.mean((q - t_y) ** 2))) for q in (with_fold, skipped)]
    print("RMSE with fold-in %.4f, with the new id skipped %.4f" % tuple(rmse))
    assert rmse[0] < rmse[1]

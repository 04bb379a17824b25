"""Top-N recommendation (include/vbfm.h "candidate sets and recommendation"): Model.candidates /
Model.recommend and bin/libFM -candidates against the EXISTING scorer -- every (context, candidate)
pair expanded on the host into one row holding both sets of entries, scored with
Model.score(order="exact", clip=False) and ranked in numpy.

Tolerance: TOL = 1e-9 * max(1, max_j |ref(c, j)|) per context, the project's bound for a reordered
fp64 sum (REL in tests/test_score_gpu.py): the pair expression sums the same products in another
order than the scorer of the merged row. Everything that compares the code with itself (chunk sizes,
slice counts, a reused candidate set, clip against no clip, duplicates) is bit for bit.

Models are written with Model.write_params from numpy arrays; nothing is trained.
"""
import os
import subprocess

import numpy as np
import pytest

import vbfm
from conftest import GOLDEN, ROOT
from recommend_cases import ALS, D_SYNTH, F, MCMC_DRAW, VB, bits, candidates, contexts, expand, make_model, same

pytestmark = pytest.mark.gpu
REL = 1e-9
CLI = os.path.join(ROOT, "scalable-variational-bayesian-factorization-machine_amd", "bin", "libFM")
# the pair kernel's geometry (csrc/vbfm_recommend.hip): a wave owns REC_CTX contexts, a workgroup
# REC_TILE_B (half of it when topn > 64); a wave step takes REC_STEP candidates, slices are whole steps
REC_CTX, REC_TILE_B, REC_STEP = 16, 64, 128


def reference(m, ctx, cand, clip=False, unknown_ids="refuse"):
    B, M = len(ctx[0]) - 1, len(cand[0]) - 1
    if B * M == 0:
        return np.zeros((B, M))
    return m.score(expand(ctx, cand), order="exact", clip=clip, unknown_ids=unknown_ids).reshape(B, M)


def check(res, ref, topn, excl=None, label=""):
    """The issue's checks of one result against the reference scores ref [B, M]."""
    idx, score, count = res
    B, M = ref.shape
    assert idx.shape == (B, topn) and score.shape == (B, topn) and count.shape == (B,)
    for c in range(B):
        allowed = np.isfinite(ref[c])
        if excl is not None:
            allowed[np.asarray(excl[c], dtype=np.int64)] = False
        n = int(count[c])
        assert n == min(topn, int(allowed.sum())), (label, c, n, int(allowed.sum()))
        got, sc = idx[c, :n].astype(np.int64), score[c, :n]
        assert np.all(idx[c, n:] == -1) and np.all(np.isnan(score[c, n:])), (label, c)
        assert len(set(got.tolist())) == n and np.all((got >= 0) & (got < M)) and np.all(allowed[got]), (label, c)
        if n == 0:
            continue
        fin = ref[c][np.isfinite(ref[c])]
        tol = REL * max(1.0, float(np.max(np.abs(fin))) if fin.size else 1.0)
        err = np.max(np.abs(sc - ref[c, got]))
        kth = np.sort(ref[c, allowed])[::-1][n - 1]
        print("%s ctx %d: max |score - ref| %.3e (tol %.3e), worst margin to the reference's cut %.3e" % (
            label, c, err, tol, float(np.min(ref[c, got] - kth))))
        assert err <= tol, (label, c, err, tol)
        assert np.all(ref[c, got] >= kth - 2 * tol), (label, c)
        assert np.all(sc[:-1] >= sc[1:]), (label, c)
        ties = sc[:-1] == sc[1:]
        assert np.all(got[:-1][ties] < got[1:][ties]), (label, c)


# ---- 1. every k, kind, tile and slice edge ---------------------------------------------------
# k rotates through the G / KP boundaries of the preparation kernel; B through the wave's and the
# workgroup's context tile +-1; M through the candidate step +-1 and M < topn; topn through the three
# list capacities (16, 64, 128) of the pair kernel
SHAPES = [
    # k, k0, k1, kind, task, B, M, topn
    (0, 1, 1, VB, "r", 17, 129, 10),
    (1, 0, 1, ALS, "r", 1, 1, 1),
    (7, 1, 0, VB, "r", REC_CTX - 1, REC_STEP - 1, 10),
    (8, 1, 1, MCMC_DRAW, "c", REC_CTX, REC_STEP, 128),
    (9, 0, 0, VB, "r", REC_CTX + 1, REC_STEP + 1, 1),
    (33, 1, 1, ALS, "r", REC_TILE_B - 1, 2 * REC_STEP + 1, 10),
    (64, 1, 1, VB, "r", REC_TILE_B, 5, 10),            # M < topn: short lists, padding
    (65, 0, 1, MCMC_DRAW, "c", REC_TILE_B + 1, 2 * REC_STEP - 1, 128),
    (100, 1, 1, VB, "r", 3, 100, 128),                 # M < topn
    (100, 1, 0, ALS, "r", 1, 3 * REC_STEP, 64),
    (16, 1, 1, ALS, "r", REC_TILE_B // 2 + 1, REC_STEP + 1, 100),   # the two-wave workgroup's tile + 1
]


@pytest.mark.parametrize("k,k0,k1,kind,task,B,M,topn", SHAPES)
def test_ranking_matches_the_scorer_of_the_merged_rows(tmp_path, k, k0, k1, kind, task, B, M, topn):
    m = make_model(tmp_path, kind, k, k0, k1, task=task)
    ctx, cand = contexts(B), candidates(M)
    ref = reference(m, ctx, cand)
    cs = m.candidates(cand)
    assert len(cs) == M
    res = m.recommend(ctx, cs, topn, clip=False)
    check(res, ref, topn, label="k=%d B=%d M=%d topn=%d" % (k, B, M, topn))
    st = m.last_recommend_stats
    assert st["pairs"] == B * M and st["nonfinite_pairs"] == 0 and st["n_chunks"] == 1
    cs.close()
    m.close()


# ---- 2. the total order -----------------------------------------------------------------------
def test_duplicate_candidates_tie_bit_for_bit_and_the_lower_index_wins(tmp_path):
    m = make_model(tmp_path, VB, 9, 1, 1)
    rp, f, v = candidates(40)
    lo, hi = 7, 31                                       # row hi becomes a copy of row lo
    rows = [(f[int(rp[j]):int(rp[j + 1])], v[int(rp[j]):int(rp[j + 1])]) for j in range(40)]
    rows[hi] = rows[lo]
    rp2 = np.zeros(41, dtype=np.uint64)
    np.cumsum([len(r[0]) for r in rows], out=rp2[1:])
    cand = (rp2, np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows]))
    cs = m.candidates(cand)
    ctx = contexts(3)
    idx, score, count = m.recommend(ctx, cs, 40, clip=False)
    assert np.all(count == 40)
    for c in range(3):
        p = int(np.nonzero(idx[c] == lo)[0][0])
        assert idx[c, p + 1] == hi and bits(score[c, p]) == bits(score[c, p + 1])
        # only one of the two fits at rank p + 1: the lower index is kept
        one = (ctx[0][c:c + 2] - ctx[0][c], ctx[1][int(ctx[0][c]):int(ctx[0][c + 1])], ctx[2][int(ctx[0][c]):int(ctx[0][c + 1])])
        i1, s1, c1 = m.recommend(one, cs, p + 1, clip=False)
        assert c1[0] == p + 1 and i1[0, p] == lo and hi not in i1[0].tolist()
        assert np.array_equal(i1[0], idx[c, :p + 1]) and np.array_equal(bits(s1[0]), bits(score[c, :p + 1]))
    cs.close()
    m.close()


# ---- 3. geometry independence -----------------------------------------------------------------
def test_results_do_not_depend_on_chunks_slices_or_reuse(tmp_path, monkeypatch):
    m = make_model(tmp_path, ALS, 33, 1, 1)
    B, M, topn = REC_TILE_B + 5, 3 * REC_STEP + 9, 10
    ctx, cand = contexts(B), candidates(M)
    excl = [np.arange(c % 4, M, 7, dtype=np.uint32) if c % 3 else np.zeros(0, dtype=np.uint32) for c in range(B)]
    cs = m.candidates(cand)
    monkeypatch.delenv("VBFM_REC_SLICES", raising=False)
    base = m.recommend(ctx, cs, topn, exclude=excl)
    ref = reference(m, ctx, cand)
    check(m.recommend(ctx, cs, topn, exclude=excl, clip=False), ref, topn, excl, "geometry base")
    assert m.last_recommend_stats["n_chunks"] == 1
    again = m.recommend(ctx, cs, topn, exclude=excl)           # the candidate set reused
    assert same(base, again)
    row_bytes = 8 + F * 8
    for chunk_bytes, chunks in ((1, B), (8 + 3 * row_bytes, (B + 2) // 3), (8 + 64 * row_bytes, 2), (1 << 20, 1)):
        got = m.recommend(ctx, cs, topn, exclude=excl, chunk_bytes=chunk_bytes)
        assert m.last_recommend_stats["n_chunks"] == chunks, (chunk_bytes, m.last_recommend_stats)
        assert same(base, got), chunk_bytes
    for slices in ("1", "2", "7", "100"):                      # read at every call; > 64: the wide merge kernel
        monkeypatch.setenv("VBFM_REC_SLICES", slices)
        assert same(base, m.recommend(ctx, cs, topn, exclude=excl)), slices
        assert same(base, m.recommend(ctx, cs, topn, exclude=excl, chunk_bytes=8 + 3 * row_bytes)), slices
    for big in (64, 100):                                      # the other list capacities' workgroups, with exclusions
        monkeypatch.delenv("VBFM_REC_SLICES")
        want = m.recommend(ctx, cs, big, exclude=excl, clip=False)
        check(want, ref, big, excl, "geometry topn=%d" % big)
        monkeypatch.setenv("VBFM_REC_SLICES", "7")
        assert same(want, m.recommend(ctx, cs, big, exclude=excl, clip=False)), big
    cs.close()
    m.close()


# ---- 4. exclusions ----------------------------------------------------------------------------
def test_exclusions(tmp_path):
    m = make_model(tmp_path, VB, 8, 1, 1)
    B, M, topn = 6, REC_STEP + 20, 10
    ctx, cand = contexts(B), candidates(M)
    ref = reference(m, ctx, cand)
    top = np.argsort(-ref, axis=1, kind="stable")
    excl = [np.zeros(0, dtype=np.uint32),                      # nothing
            np.sort(top[1, :5]).astype(np.uint32),             # the reference's top entries
            np.arange(M, dtype=np.uint32),                     # every candidate
            np.sort(top[3, :topn + 3]).astype(np.uint32),
            np.zeros(0, dtype=np.uint32),
            np.sort(top[5, ::2]).astype(np.uint32)]
    cs = m.candidates(cand)
    res = m.recommend(ctx, cs, topn, exclude=excl, clip=False)
    check(res, ref, topn, excl, "exclusions")
    assert res[2][2] == 0 and np.all(res[0][2] == -1)
    assert m.last_recommend_stats["excluded_hits"] >= 5 + M
    # the (ptr, idx) form is the same call
    ptr = np.zeros(B + 1, dtype=np.uint64)
    np.cumsum([len(e) for e in excl], out=ptr[1:])
    assert same(res, m.recommend(ctx, cs, topn, exclude=(ptr, np.concatenate(excl)), clip=False))
    bad = [e.copy() for e in excl]
    bad[3] = bad[3][::-1].copy()
    with pytest.raises(vbfm.VbfmError, match=r"context row 3 is not sorted"):
        m.recommend(ctx, cs, topn, exclude=bad)
    bad = [e.copy() for e in excl]
    bad[4] = np.array([2, M], dtype=np.uint32)
    with pytest.raises(vbfm.VbfmError, match=r"context row 4 holds candidate index %d" % M):
        m.recommend(ctx, cs, topn, exclude=bad)
    cs.close()
    m.close()


# ---- 5. non-finite pairs ----------------------------------------------------------------------
def test_a_nonfinite_candidate_is_never_returned(tmp_path):
    B, M, topn, special = 5, REC_STEP + 3, 10, 77
    ctx = contexts(B)
    rp, f, v = candidates(M)
    f = f.copy()
    f[int(rp[special])] = D_SYNTH - 1                          # the only row that holds id 250; no context does
    cand = (rp, f, v)

    def inf_weight(p):
        p["w"][D_SYNTH - 1] = np.inf

    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    m_inf = make_model(tmp_path / "a", ALS, 7, 1, 1, edit=inf_weight)
    m_fin = make_model(tmp_path / "b", ALS, 7, 1, 1)
    cs_inf, cs_fin = m_inf.candidates(cand), m_fin.candidates(cand)
    res = m_inf.recommend(ctx, cs_inf, topn, clip=False)
    assert m_inf.last_recommend_stats["nonfinite_pairs"] == B
    assert special not in res[0].ravel().tolist()
    check(res, reference(m_inf, ctx, cand), topn, label="inf weight")
    # the other results: the finite model with that candidate excluded
    want = m_fin.recommend(ctx, cs_fin, topn, exclude=[np.array([special], dtype=np.uint32)] * B, clip=False)
    assert m_fin.last_recommend_stats["nonfinite_pairs"] == 0
    assert same(res, want)
    for h in (cs_inf, cs_fin, m_inf, m_fin):
        h.close()


# ---- 6. refusals and unknown ids --------------------------------------------------------------
def test_refusals(tmp_path):
    m = make_model(tmp_path, VB, 8, 1, 1)
    ctx, cand = contexts(4), candidates(20)
    cs = m.candidates(cand)
    for topn in (0, vbfm.REC_MAX_TOPN + 1):
        with pytest.raises(vbfm.VbfmError, match=r"topn = %d is outside 1 \.\. 128" % topn):
            m.recommend(ctx, cs, topn)
    (tmp_path / "other").mkdir()
    other = make_model(tmp_path / "other", VB, 8, 1, 1)
    with pytest.raises(vbfm.VbfmError, match="made from another model"):
        other.recommend(ctx, cs, 5)
    big = make_model(tmp_path, ALS, 257, 1, 1, D=8)
    with pytest.raises(vbfm.VbfmError, match=r"num_factor = 257 is beyond the limit of 256"):
        big.candidates((np.array([0, 1], dtype=np.uint64), np.array([1], dtype=np.uint32), np.ones(1, dtype=np.float32)))
    for h in (cs, m, other, big):
        h.close()


def test_unknown_ids_refuse_and_skip(tmp_path):
    m = make_model(tmp_path, VB, 9, 1, 1)
    B, M, topn = 5, 30, 10
    rp, f, v = contexts(B)
    f = f.copy()
    f[int(rp[2]) + 1] = D_SYNTH + 40                           # context row 2 holds an id the model lacks
    ctx = (rp, f, v)
    jrp, jf, jv = candidates(M)
    jf = jf.copy()
    jf[int(jrp[4])] = D_SYNTH + 9                              # and so does candidate row 4
    cand = (jrp, jf, jv)
    with pytest.raises(vbfm.VbfmError) as scorer:
        m.score(cand, clip=False)
    with pytest.raises(vbfm.VbfmError) as e:
        m.candidates(cand)
    assert str(e.value) == str(scorer.value) and "row 4 holds feature id %d" % (D_SYNTH + 9) in str(e.value)
    cs = m.candidates(cand, unknown_ids="skip")
    with pytest.raises(vbfm.VbfmError) as scorer:
        m.score(ctx, clip=False)
    with pytest.raises(vbfm.VbfmError) as e:
        m.recommend(ctx, cs, topn)
    assert str(e.value) == str(scorer.value) and "row 2 holds feature id %d" % (D_SYNTH + 40) in str(e.value)
    res = m.recommend(ctx, cs, topn, clip=False, unknown_ids="skip")
    check(res, reference(m, ctx, cand, unknown_ids="skip"), topn, label="skip")
    cs.close()
    m.close()


# ---- 7. clip -------------------------------------------------------------------------------
def test_clip_is_applied_to_the_survivors_and_never_changes_the_ranking(tmp_path):
    B, M, topn = 9, REC_STEP + 7, 10
    ctx, cand = contexts(B), candidates(M)
    m = make_model(tmp_path, VB, 8, 1, 1, mn=-0.25, mx=0.5)    # a range the best pairs leave
    cs = m.candidates(cand)
    raw = m.recommend(ctx, cs, topn, clip=False)
    clipped = m.recommend(ctx, cs, topn, clip=True)
    assert np.array_equal(raw[0], clipped[0]) and np.array_equal(raw[2], clipped[2])
    assert np.any(raw[1] > 0.5)
    assert np.array_equal(bits(clipped[1]), bits(np.clip(raw[1], np.float32(-0.25), np.float32(0.5))))
    cs.close()
    m.close()
    mc = make_model(tmp_path, MCMC_DRAW, 8, 1, 1, task="c")
    cs = mc.candidates(cand)
    raw = mc.recommend(ctx, cs, topn, clip=False)
    prob = mc.recommend(ctx, cs, topn, clip=True)
    assert np.array_equal(raw[0], prob[0]) and np.array_equal(raw[2], prob[2])
    want = reference(mc, ctx, cand, clip=True)                 # Phi(yhat) of the merged rows
    err = np.max(np.abs(prob[1] - np.take_along_axis(want, prob[0].astype(np.int64), axis=1)))
    print("task c: max |Phi(raw) - Model.score(clip=True)| %.3e" % err)
    assert err <= REL * 1.0 and np.all((prob[1] >= 0) & (prob[1] <= 1))
    cs.close()
    mc.close()


# ---- 8. the CLI -------------------------------------------------------------------------------
def test_cli_round_trip_and_flag_refusals(tmp_path):
    d = os.path.join(GOLDEN, "tiny")
    tr, te = os.path.join(d, "train.libfm"), os.path.join(d, "test.libfm")
    items, users = vbfm.DataSubset.load(tr), vbfm.DataSubset.load(te)
    D = vbfm.num_all_attribute(items, users)
    m = make_model(tmp_path, VB, 3, 1, 1, D=D, mn=float(items.min_target), mx=float(items.max_target))
    mfile = [str(p) for p in tmp_path.iterdir() if str(p).endswith(".vbfm")][0]
    B, M, topn = users.num_cases, items.num_cases, 3
    rng = np.random.default_rng(9)
    excl = [rng.permutation(M)[:rng.integers(0, 4)] for _ in range(B)]
    excl[0] = np.array([2, 0, 2, 1]) % M                       # any order, with a duplicate
    with open(tmp_path / "ex", "w") as fh:
        for e in excl:
            fh.write(" ".join(str(int(x)) for x in e) + "\n")
    r = subprocess.run([CLI, "-load_model", mfile, "-test", te, "-candidates", tr, "-topn", str(topn), "-out", "rec",
                        "-exclude", "ex"], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    cs = m.candidates(items)
    idx, score, count = m.recommend(users, cs, topn, exclude=[np.unique(e).astype(np.uint32) for e in excl])
    want = [" ".join("%d:%.17g" % (idx[c, e], score[c, e]) for e in range(count[c])) for c in range(B)]
    got = open(tmp_path / "rec").read().split("\n")
    assert got[-1] == "" and got[:-1] == want
    assert count.max() > 0
    cs.close()
    m.close()
    base = [CLI, "-load_model", mfile, "-test", te, "-out", "o"]
    for extra, msg in ((["-topn", "3"], "-topn needs -candidates"),
                       (["-candidates", tr, "-topn", "3", "-out_var", "v"], "-out_var does not apply to -candidates"),
                       (["-exclude", "ex"], "-exclude needs -candidates"),
                       (["-candidates", tr], "-candidates needs -topn")):
        r = subprocess.run(base + extra, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
        assert msg in r.stderr, (extra, r.stderr[-500:])
    r = subprocess.run([CLI, "-task", "r", "-train", tr, "-test", te, "-candidates", tr, "-topn", "3"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert "-candidates, -topn and -exclude belong to -load_model" in r.stderr

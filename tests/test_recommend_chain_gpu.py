"""Top-N from a chain of draws (include/vbfm.h "ranking a chain of draws"): Model.candidates_chain /
Model.recommend_chain and bin/libFM on a chain file against the EXISTING scorer -- every (context,
candidate) pair expanded on the host into one row holding both sets of entries, scored with
Model.score(variance=True, order="exact", clip=False) of the same chain model (the mean and the spread
over the draws), and key = mean + beta * sqrt(var + noise * mean(1 / alpha_s)) formed and ranked in
numpy.

Tolerances (tests/recommend_chain_cases.py tolerances): per context tol_m = 1e-9 max(1, max|mean|) and
tol_v = 1e-9 max(1, max var), the project's bound for a reordered fp64 sum; per pair tol_key = tol_m +
|beta| min(sqrt(tol_v), tol_v / sqrt(var + na)). At most 5 % of a case's pairs may fall on the loose
sqrt(tol_v) branch (var + na < 1e4 tol_v); tests/test_recommend_chain_cpu.py shows on a numpy FM that
the case table keeps that. Cases of one draw assert var == 0 and, without noise, key's bits in score.
Everything that compares the code with itself or with Model.recommend of one draw is bit for bit.

A chain of 5 copies of one draw, clip=True: the documented score is ((((p + p) + p) + p) + p) / 5, which
is not p in about 12 % of doubles, so that comparison restates the sum in numpy (bit for bit) instead
of expecting Model.recommend's p; idx and count, and everything with clip=False, are Model.recommend's.

Largest errors seen on an MI355X (the prints below; DESIGN.md §16 quotes them): 1.94e-5 of tol_m in
score, 1.93e-5 of tol_v in var, 5.4e-6 of tol_key in key; at most 1.30 % of a case's pairs on the loose
branch.
"""
import os
import subprocess

import numpy as np
import pytest

import vbfm
from conftest import GOLDEN, ROOT
from recommend_cases import ALS, D_SYNTH, F, MCMC_DRAW, VB, bits, candidates, contexts, expand, make_model, same
from recommend_chain_cases import (CASE_IDS, CASES, CHAIN_TILE_B, LOOSE_SHARE, REC_STEP, chain_draws, draw_model, make_chain,
                                   noise_term, tolerances, write_chain)

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "scalable-variational-bayesian-factorization-machine_amd", "bin", "libFM")


def reference(m, ctx, cand, clip=False):
    """(mean, var) [B, M] of the merged rows over the chain's draws, by the existing scorer."""
    B, M = len(ctx[0]) - 1, len(cand[0]) - 1
    if B * M == 0:
        return np.zeros((B, M)), np.zeros((B, M))
    mean, var = m.score(expand(ctx, cand), variance=True, order="exact", clip=clip)
    return mean.reshape(B, M), var.reshape(B, M)


def ref_key(mean, var, beta, na):
    with np.errstate(invalid="ignore"):
        return mean + beta * np.sqrt(var + na)


WORST = {"score": 0.0, "var": 0.0, "key": 0.0}


def check(res, ref, beta, na, topn, S, excl=None, label=""):
    """The checks of one clip=False result against the reference (mean, var) [B, M]; returns the share of
    the pairs on the loose branch of tol_key."""
    idx, key, score, var, count = res
    mean, rv = ref
    B, M = mean.shape
    rk = ref_key(mean, rv, beta, na)
    tol_m, tol_v, tol_key, loose = tolerances(mean, rv, na, beta)
    assert idx.shape == (B, topn) and count.shape == (B,)
    assert key.shape == (B, topn) and score.shape == (B, topn) and var.shape == (B, topn)
    for c in range(B):
        allowed = np.isfinite(mean[c]) & np.isfinite(rv[c])
        if excl is not None:
            allowed[np.asarray(excl[c], dtype=np.int64)] = False
        n = int(count[c])
        assert n == min(topn, int(allowed.sum())), (label, c, n, int(allowed.sum()))
        got = idx[c, :n].astype(np.int64)
        assert np.all(idx[c, n:] == -1), (label, c)
        for a in (key, score, var):
            assert np.all(np.isnan(a[c, n:])) and np.all(np.isfinite(a[c, :n])), (label, c)
        assert len(set(got.tolist())) == n and np.all((got >= 0) & (got < M)) and np.all(allowed[got]), (label, c)
        if n == 0:
            continue
        tm, tv, tk = float(tol_m[c, 0]), float(tol_v[c, 0]), tol_key[c]
        e_m = float(np.max(np.abs(score[c, :n] - mean[c, got])))
        e_v = float(np.max(np.abs(var[c, :n] - rv[c, got])))
        d_k = np.abs(key[c, :n] - rk[c, got])
        e_k = float(np.max(d_k / tk[got]))
        kth = np.sort(rk[c, allowed])[::-1][n - 1]
        for name, e in (("score", e_m / tm), ("var", e_v / tv), ("key", e_k)):
            WORST[name] = max(WORST[name], e)
        print("%s ctx %d: |score - ref| %.3e (tol %.3e), |var - ref| %.3e (tol %.3e), worst |key - ref| / tol_key %.3e, "
              "worst margin to the reference's cut %.3e" % (label, c, e_m, tm, e_v, tv, e_k, float(np.min(rk[c, got] - kth))))
        assert e_m <= tm and e_v <= tv and np.all(d_k <= tk[got]), (label, c, e_m, tm, e_v, tv, e_k)
        assert np.all(rk[c, got] >= kth - 2 * tk[got]), (label, c)
        kc = key[c, :n]
        assert np.all(kc[:-1] >= kc[1:]), (label, c)
        ties = kc[:-1] == kc[1:]
        assert np.all(got[:-1][ties] < got[1:][ties]), (label, c)
        if S == 1:
            assert np.all(var[c, :n] == 0.0), (label, c)
            if na == 0.0:
                assert np.array_equal(bits(key[c, :n]), bits(score[c, :n])), (label, c)
    share = float(loose.mean()) if loose.size else 0.0
    print("%s: %.2f %% of the pairs on the loose branch of tol_key; worst error / tolerance so far: score %.3g, var %.3g, "
          "key %.3g" % (label, 100 * share, WORST["score"], WORST["var"], WORST["key"]))
    if S >= 2:
        assert share <= LOOSE_SHARE, (label, share)
    return share


# ---- 1. every k, S, tile and slice edge against the scorer ----------------------------------------
@pytest.mark.parametrize("k,k0,k1,S,B,M,topn,beta,noise,task", CASES, ids=CASE_IDS)
def test_ranking_matches_the_scorer_of_the_merged_rows(tmp_path, k, k0, k1, S, B, M, topn, beta, noise, task):
    m, _, draws = make_chain(tmp_path, k, k0, k1, S, task=task)
    assert m.num_draws == S
    ctx, cand = contexts(B), candidates(M)
    ref = reference(m, ctx, cand)
    cs = m.candidates_chain(cand)
    assert len(cs) == M
    res = m.recommend_chain(ctx, cs, topn, beta, noise=bool(noise), clip=False)
    check(res, ref, beta, noise_term(draws, noise), topn, S,
          label="k=%d S=%d B=%d M=%d topn=%d beta=%g noise=%d task=%s" % (k, S, B, M, topn, beta, noise, task))
    st = m.last_recommend_stats
    assert st["pairs"] == B * M and st["nonfinite_pairs"] == 0 and st["n_chunks"] == 1
    cs.close()
    m.close()


@pytest.mark.parametrize("k,S,task", [(8, 9, "r"), (9, 17, "c")])
def test_clip_changes_the_score_only(tmp_path, k, S, task):
    B, M, topn, beta = 9, REC_STEP + 7, 10, 0.5
    ctx, cand = contexts(B), candidates(M)
    m, _, draws = make_chain(tmp_path, k, 1, 1, S, task=task, mn=-0.25, mx=0.5)   # a range the best pairs leave
    cs = m.candidates_chain(cand)
    raw = m.recommend_chain(ctx, cs, topn, beta, clip=False)
    clipped = m.recommend_chain(ctx, cs, topn, beta, clip=True)
    for i in (0, 1, 3, 4):
        assert np.array_equal(bits(raw[i]), bits(clipped[i])) if raw[i].dtype == np.float64 else np.array_equal(raw[i], clipped[i])
    ref = reference(m, ctx, cand)
    check(raw, ref, beta, 0.0, topn, S, label="clip=False k=%d task=%s" % (k, task))
    want = reference(m, ctx, cand, clip=True)[0]
    tol_m = tolerances(ref[0], ref[1], 0.0, beta)[0]
    assert np.all(clipped[4] == topn)
    got = np.take_along_axis(want, clipped[0].astype(np.int64), axis=1)
    err = np.abs(clipped[2] - got)
    print("clip=True k=%d task=%s: worst |score - ref| / tol_m %.3e" % (k, task, float(np.max(err / tol_m))))
    assert np.all(err <= tol_m)
    assert not np.array_equal(bits(raw[2]), bits(clipped[2]))     # the link or the clip did something
    if task == "c":
        assert np.all((clipped[2] >= 0.0) & (clipped[2] <= 1.0))
    else:
        assert np.any(raw[2] > 0.5) and np.all(clipped[2] <= np.float32(0.5))
    cs.close()
    m.close()


# ---- 2. one draw, or copies of one draw, is Model.recommend of that draw, bit for bit ------------------
@pytest.mark.parametrize("copies", [1, 5])
def test_one_draw_is_recommend_of_that_draw_bit_for_bit(tmp_path, copies):
    k, topn = 9, 10
    B, M = CHAIN_TILE_B + 3, 2 * REC_STEP + 5
    ctx, cand = contexts(B), candidates(M)
    draws = chain_draws(k, 1) * copies
    path = write_chain(tmp_path, k, 1, 1, draws, mn=-0.25, mx=0.5)
    chain = vbfm.Model.load(path)
    one = draw_model(tmp_path, path, 0)
    assert one.info["kind"] == MCMC_DRAW and chain.num_draws == copies
    plain, cs = one.candidates(cand), chain.candidates_chain(cand)
    for clip in (False, True):
        want = one.recommend(ctx, plain, topn, clip=clip)
        got = chain.recommend_chain(ctx, cs, topn, 0.0, clip=clip)
        assert np.array_equal(want[0], got[0]) and np.array_equal(want[2], got[4])
        assert np.all(got[3][got[0] >= 0] == 0.0)                 # var
        score = want[1]
        if clip and copies > 1:                                   # the documented sum over equal p_s (module docstring)
            acc = np.zeros_like(score)
            for _ in range(copies):
                acc = acc + score
            score = np.clip(acc / float(copies), np.float32(-0.25), np.float32(0.5))
        assert np.array_equal(bits(score), bits(got[2])), (copies, clip)
        if not clip:
            assert np.array_equal(bits(got[1]), bits(got[2]))     # key == score
    # noise = 0: sd is 0 for every pair, so any beta returns what beta = 0 returns
    base = chain.recommend_chain(ctx, cs, topn, 0.0, clip=False)
    for beta in (2.0, -1.0):
        assert same(base, chain.recommend_chain(ctx, cs, topn, beta, clip=False)), beta
    for h in (plain, cs, one, chain):
        h.close()


# ---- 3. geometry independence -----------------------------------------------------------------
def test_results_do_not_depend_on_chunks_slices_or_reuse(tmp_path, monkeypatch):
    k, S = 33, 3
    m, _, draws = make_chain(tmp_path, k, 1, 1, S)
    B, M, topn = 2 * CHAIN_TILE_B + 5, 3 * REC_STEP + 9, 10
    ctx, cand = contexts(B), candidates(M)
    excl = [np.arange(c % 4, M, 7, dtype=np.uint32) if c % 3 else np.zeros(0, dtype=np.uint32) for c in range(B)]
    cs = m.candidates_chain(cand)
    monkeypatch.delenv("VBFM_REC_SLICES", raising=False)
    call = lambda **kw: m.recommend_chain(ctx, cs, topn, 2.0, noise=True, exclude=excl, **kw)
    base = call()
    check(call(clip=False), reference(m, ctx, cand), 2.0, noise_term(draws, 1), topn, S, excl, "geometry base")
    assert m.last_recommend_stats["n_chunks"] == 1
    assert same(base, call())                                   # the candidate set reused
    row_bytes, sums = 8 + F * 8, S * (k + 1) * 8                # a staged row; its prepared sums
    assert 8 + B * row_bytes < 8 + 20 * (row_bytes + sums)      # the staged rows alone fit the second budget at once
    # 1 byte: chunks of one wave's tile; then the prepared sums cut the chunk at 20 rows; then one chunk
    for chunk_bytes, chunks in ((1, (B + 7) // 8), (8 + 20 * (row_bytes + sums), (B + 19) // 20), (1 << 20, 1)):
        got = call(chunk_bytes=chunk_bytes)
        assert m.last_recommend_stats["n_chunks"] == chunks, (chunk_bytes, m.last_recommend_stats)
        assert same(base, got), chunk_bytes
    assert (B + 19) // 20 > 1
    for slices in ("1", "3", "64"):                             # read at every call
        monkeypatch.setenv("VBFM_REC_SLICES", slices)
        assert same(base, call()), slices
        assert same(base, call(chunk_bytes=1)), slices
    monkeypatch.delenv("VBFM_REC_SLICES")
    for big in (64, 128):                                       # the other list capacities
        want = m.recommend_chain(ctx, cs, big, -1.0, exclude=excl)
        monkeypatch.setenv("VBFM_REC_SLICES", "3")
        assert same(want, m.recommend_chain(ctx, cs, big, -1.0, exclude=excl, chunk_bytes=1)), big
        monkeypatch.delenv("VBFM_REC_SLICES")
    cs.close()
    m.close()


# ---- 4. the total order -----------------------------------------------------------------------
def test_duplicate_candidates_tie_bit_for_bit_and_the_lower_index_wins(tmp_path):
    m, _, _ = make_chain(tmp_path, 9, 1, 1, 3)
    rp, f, v = candidates(40)
    lo, hi = 7, 31                                              # row hi becomes a copy of row lo
    rows = [(f[int(rp[j]):int(rp[j + 1])], v[int(rp[j]):int(rp[j + 1])]) for j in range(40)]
    rows[hi] = rows[lo]
    rp2 = np.zeros(41, dtype=np.uint64)
    np.cumsum([len(r[0]) for r in rows], out=rp2[1:])
    cand = (rp2, np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows]))
    cs = m.candidates_chain(cand)
    ctx = contexts(3)
    idx, key, score, var, count = m.recommend_chain(ctx, cs, 40, 2.0, clip=False)
    assert np.all(count == 40)
    for c in range(3):
        p = int(np.nonzero(idx[c] == lo)[0][0])
        assert idx[c, p + 1] == hi
        for a in (key, score, var):
            assert bits(a[c, p]) == bits(a[c, p + 1])
        # only one of the two fits at rank p + 1: the lower index is kept
        one = (ctx[0][c:c + 2] - ctx[0][c], ctx[1][int(ctx[0][c]):int(ctx[0][c + 1])], ctx[2][int(ctx[0][c]):int(ctx[0][c + 1])])
        r1 = m.recommend_chain(one, cs, p + 1, 2.0, clip=False)
        assert r1[4][0] == p + 1 and r1[0][0, p] == lo and hi not in r1[0][0].tolist()
        assert np.array_equal(r1[0][0], idx[c, :p + 1]) and np.array_equal(bits(r1[1][0]), bits(key[c, :p + 1]))
    # an excluded index is never returned, the best candidate included
    excl = [np.sort(idx[c, :5]).astype(np.uint32) for c in range(3)]
    r2 = m.recommend_chain(ctx, cs, 40, 2.0, exclude=excl, clip=False)
    for c in range(3):
        assert r2[4][c] == 35 and not set(excl[c].tolist()) & set(r2[0][c, :35].tolist())
        assert np.array_equal(r2[0][c, :35], idx[c, 5:]) and np.array_equal(bits(r2[1][c, :35]), bits(key[c, 5:]))
    assert m.last_recommend_stats["excluded_hits"] >= 15
    cs.close()
    m.close()


# ---- 5. a non-finite draw ---------------------------------------------------------------------
def edit_nan_draw_1(draws):
    draws[1]["w"][D_SYNTH - 1] = np.nan


def edit_inf_draw_0(draws):
    draws[0]["w"][D_SYNTH - 1] = np.inf


@pytest.mark.parametrize("edit", [edit_nan_draw_1, edit_inf_draw_0])
def test_a_candidate_that_is_not_finite_in_one_draw_is_never_returned(tmp_path, edit):
    B, M, topn, special, S = 5, REC_STEP + 3, 10, 77, 3
    ctx = contexts(B)
    rp, f, v = candidates(M)
    f = f.copy()
    f[int(rp[special])] = D_SYNTH - 1                           # the only row that holds id 250; no context does
    cand = (rp, f, v)
    m_bad, _, draws = make_chain(tmp_path, 7, 1, 1, S, edit=edit, name="bad")
    m_fin, _, _ = make_chain(tmp_path, 7, 1, 1, S, name="fin")
    cs_bad, cs_fin = m_bad.candidates_chain(cand), m_fin.candidates_chain(cand)
    ref = reference(m_bad, ctx, cand)
    bad = ~np.isfinite(ref[0])
    assert np.all(bad[:, special]) and bad.sum() == B          # the reference agrees: that column and nothing else
    res = m_bad.recommend_chain(ctx, cs_bad, topn, 2.0, clip=False)
    assert m_bad.last_recommend_stats["nonfinite_pairs"] == B
    assert special not in res[0].ravel().tolist()
    # the other results: the finite model with that candidate excluded
    want = m_fin.recommend_chain(ctx, cs_fin, topn, 2.0, exclude=[np.array([special], dtype=np.uint32)] * B, clip=False)
    assert m_fin.last_recommend_stats["nonfinite_pairs"] == 0
    assert same(res, want)
    for h in (cs_bad, cs_fin, m_bad, m_fin):
        h.close()


# ---- 6. refusals ----------------------------------------------------------------------------
def test_refusals(tmp_path):
    ctx, cand = contexts(4), candidates(20)
    chain, _, _ = make_chain(tmp_path, 8, 1, 1, 2)
    cs = chain.candidates_chain(cand)
    for kind, name in ((VB, "VBFM_MODEL_VB"), (ALS, "VBFM_MODEL_ALS"), (MCMC_DRAW, "VBFM_MODEL_MCMC_DRAW")):
        pm = make_model(tmp_path, kind, 8, 1, 1)
        with pytest.raises(vbfm.VbfmError, match=r"vbfm_candidates_create_chain: a model of kind %s holds one set of parameters, "
                                                 r"not a chain.*vbfm_candidates_create / vbfm_recommend" % name):
            pm.candidates_chain(cand)
        with pytest.raises(vbfm.VbfmError, match=r"vbfm_recommend_chain: a model of kind %s holds one set of parameters, "
                                                 r"not a chain.*vbfm_candidates_create / vbfm_recommend" % name):
            pm.recommend_chain(ctx, cs, 5)
        # a plain or variance set in recommend_chain; a chain set in recommend and recommend_ucb
        sets = [(pm.candidates(cand), r"made by vbfm_candidates_create; use vbfm_candidates_create_chain")]
        if kind == VB:
            sets.append((pm.candidates(cand, variance=True), r"made by vbfm_candidates_create_var; use vbfm_candidates_create_chain"))
        for s, msg in sets:
            with pytest.raises(vbfm.VbfmError, match=r"vbfm_recommend_chain: the candidate set holds one set of sums \(it was " + msg):
                chain.recommend_chain(ctx, s, 5)
            s.close()
        with pytest.raises(vbfm.VbfmError, match=r"vbfm_recommend: the candidate set holds the sums of a chain's 2 draws"):
            pm.recommend(ctx, cs, 5)
        with pytest.raises(vbfm.VbfmError, match=r"vbfm_recommend_ucb: the candidate set holds the sums of a chain's 2 draws"):
            pm.recommend_ucb(ctx, cs, 5, 1.0)
        pm.close()
    # the old entry points go on refusing the chain model itself
    with pytest.raises(vbfm.VbfmError, match=r"vbfm_recommend: a chain of draws \(VBFM_MODEL_MCMC_CHAIN\) is scored, not ranked"):
        chain.recommend(ctx, cs, 5)
    with pytest.raises(vbfm.VbfmError, match=r"vbfm_candidates_create: a chain of draws \(VBFM_MODEL_MCMC_CHAIN\) is scored, not ranked"):
        chain.candidates(cand)
    other, _, _ = make_chain(tmp_path, 8, 1, 1, 2, name="other")
    with pytest.raises(vbfm.VbfmError, match="made from another model"):
        other.recommend_chain(ctx, cs, 5)
    for topn in (0, vbfm.REC_MAX_TOPN + 1):
        with pytest.raises(vbfm.VbfmError, match=r"topn = %d is outside 1 \.\. 128" % topn):
            chain.recommend_chain(ctx, cs, topn)
    for beta in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(vbfm.VbfmError, match=r"beta = \S+ is not a finite number"):
            chain.recommend_chain(ctx, cs, 5, beta)
    with pytest.raises(vbfm.VbfmError, match=r"exclusion list of context row 1 is not sorted"):
        chain.recommend_chain(ctx, cs, 5, exclude=[[], [3, 2], [], []])
    with pytest.raises(vbfm.VbfmError, match=r"context row 2 holds candidate index 20, but the candidate set has 20 rows"):
        chain.recommend_chain(ctx, cs, 5, exclude=[[], [], [20], []])
    cls, _, _ = make_chain(tmp_path, 8, 1, 1, 2, task="c", name="cls")
    ccs = cls.candidates_chain(cand)
    with pytest.raises(vbfm.VbfmError, match=r"noise = 1 .* a model of task c has no noise precision"):
        cls.recommend_chain(ctx, ccs, 5, 1.0, noise=True)
    assert np.all(cls.recommend_chain(ctx, ccs, 5, 1.0)[4] == 5)
    # a set no device holds: refused from the sizes alone, both figures in the message
    big, _, _ = make_chain(tmp_path, 256, 1, 1, 64, D=2, name="big")
    M = 4_000_000
    empty = (np.zeros(M + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.float32))
    need = 64 * 257 * ((M + REC_STEP - 1) // REC_STEP * REC_STEP) * 8
    with pytest.raises(vbfm.VbfmError, match=r"vbfm_candidates_create_chain: %d candidates of num_factor = 256 and 64 draws need "
                                             r"%d bytes of device memory, \d+ are free" % (M, need)):
        big.candidates_chain(empty)
    for h in (cs, ccs, chain, other, cls, big):
        h.close()


# ---- 7. the CLI -------------------------------------------------------------------------------
def test_cli_round_trip(tmp_path):
    d = os.path.join(GOLDEN, "tiny")
    tr, te = os.path.join(d, "train.libfm"), os.path.join(d, "test.libfm")
    items, users = vbfm.DataSubset.load(tr), vbfm.DataSubset.load(te)
    D = vbfm.num_all_attribute(items, users)
    m, mfile, _ = make_chain(tmp_path, 3, 1, 1, 4, D=D, mn=float(items.min_target), mx=float(items.max_target))
    B, M, topn = users.num_cases, items.num_cases, 3
    rng = np.random.default_rng(9)
    excl = [rng.permutation(M)[:rng.integers(0, 4)] for _ in range(B)]
    with open(tmp_path / "ex", "w") as fh:
        for e in excl:
            fh.write(" ".join(str(int(x)) for x in e) + "\n")
    xs = [np.unique(e).astype(np.uint32) for e in excl]
    run = lambda args: subprocess.run([CLI] + args, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    lines = lambda idx, val, count: [" ".join("%d:%.17g" % (idx[c, e], val[c, e]) for e in range(count[c])) for c in range(B)]
    read = lambda name: open(tmp_path / name).read().split("\n")
    cs = m.candidates_chain(items)
    common = ["-load_model", mfile, "-test", te, "-candidates", tr, "-topn", str(topn), "-out", "rec", "-exclude", "ex"]
    r = run(common + ["-ucb", "1.5", "-ucb_noise", "1", "-out_rank_var", "rv"])
    assert r.returncode == 0, r.stderr[-2000:]
    idx, key, score, var, count = m.recommend_chain(users, cs, topn, 1.5, noise=True, exclude=xs)
    assert count.max() > 0
    for name, val in (("rec", score), ("rv", var)):
        got = read(name)
        assert got[-1] == "" and got[:-1] == lines(idx, val, count), name
    r = run(common)                                             # without -ucb: the chain mean
    assert r.returncode == 0, r.stderr[-2000:]
    idx0, _, score0, _, count0 = m.recommend_chain(users, cs, topn, exclude=xs)
    got = read("rec")
    assert got[-1] == "" and got[:-1] == lines(idx0, score0, count0)
    cs.close()
    m.close()
    als = make_model(tmp_path, ALS, 3, 1, 1, D=D, name="als")
    als.close()
    afile = [str(p) for p in tmp_path.iterdir() if os.path.basename(str(p)).startswith("als_")][0]
    r = run(["-load_model", afile, "-test", te, "-candidates", tr, "-topn", "3", "-out", "o", "-ucb", "1.5"])
    assert "-ucb needs a model with variances" in r.stderr and "-chain B,T" in r.stderr, r.stderr[-500:]
    assert not os.path.exists(tmp_path / "o")

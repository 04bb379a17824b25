"""Model.rank_positives / vbfm_rank_positives and bin/libFM -positives (include/vbfm.h "ranking held-out
candidates") against an oracle that needs no tolerance (tests/rank_eval_cases.py): the full key matrix of
a ranking from that ranking's own recommend call over candidate subsets of at most 128 rows, ranks and
`ranked` counted in numpy with the total order. rank, ranked and the bits of key must be EQUAL, for
every ranking, kind, tile, slice, chunk and pass count.

Models are written from numpy arrays (recommend_cases.make_model, recommend_chain_cases.make_chain);
nothing is trained.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import vbfm
from conftest import GOLDEN, ROOT
from rank_eval_cases import (EVAL_POS, equal, key_matrix, make_set, oracle, pair_bits_depend_on_the_rows_only,
                             positives_of, recommend)
from recommend_cases import ALS, D_SYNTH, F, MCMC_DRAW, VB, VB_ONLINE, bits, candidates, contexts, make_model
from recommend_chain_cases import draw_model, make_chain

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "scalable-variational-bayesian-factorization-machine_amd", "bin", "libFM")
# the counting kernels keep the pair kernels' geometry (csrc/vbfm_recommend.hip)
REC_CTX, REC_TILE_B, REC_STEP = 16, 64, 128


def counts_for(M, turn=0):
    """positives per context, cycling: none, one, a full pass, a pass + 1, two passes + 1, every candidate"""
    c = [0, 1, EVAL_POS, EVAL_POS + 1, 2 * EVAL_POS + 1, M]
    return c[turn % 6:] + c[:turn % 6]


def model_for(tmp_path, ranking, k, k0=1, k1=1, kind=None, task="r", S=3, **kw):
    if ranking == "chain":
        return make_chain(tmp_path, k, k0, k1, S, task=task, **kw)[0]
    return make_model(tmp_path, kind if kind is not None else (VB if ranking == "ucb" else ALS), k, k0, k1, task=task, **kw)


def run_case(m, ranking, B, M, counts, beta=0.0, noise=False, exclude=None, label=""):
    """One call against the oracle, its stats included; returns (got, want, K, positives)."""
    ctx, cand = contexts(B), candidates(M)
    K = key_matrix(m, ranking, ctx, cand, beta, noise)
    pos = positives_of(B, M, counts)
    if exclude is not None:                                    # a positive is never on its context's exclusion list
        pos = [np.setdiff1d(p, exclude[c]).astype(np.uint32) for c, p in enumerate(pos)]
    cs = make_set(m, ranking, cand)
    got = m.rank_positives(ctx, cs, pos, exclude=exclude, ranking=ranking, beta=beta, noise=noise)
    st = m.last_rank_stats
    cs.close()
    want = oracle(K, pos, exclude)
    equal(got, want, label)
    longest = max(len(p) for p in pos)
    assert st["pairs"] == B * M and st["positives"] == len(want[0]) and st["n_chunks"] == 1, (label, st)
    assert st["nonfinite_pairs"] == want[3] and st["nonfinite_positives"] == want[4], (label, st)
    assert st["passes"] == max(1, -(-longest // EVAL_POS)), (label, st)
    return got, want, K, pos


# ---- 0. the oracle's premise ----------------------------------------------------------------------
@pytest.mark.parametrize("ranking", ["mean", "ucb", "chain"])
def test_a_pairs_bits_depend_on_its_two_rows_only(tmp_path, ranking):
    m = model_for(tmp_path, ranking, 9)
    full = pair_bits_depend_on_the_rows_only(m, ranking, contexts(REC_CTX + 1), candidates(100), beta=1.5 if ranking != "mean" else 0.0)
    assert np.all(np.isfinite(full))
    m.close()


# ---- 1. every k, kind, tile, step and pass edge -----------------------------------------------------
# k rotates through the G / KP boundaries of the preparation kernel; B through the wave's and the
# workgroup's context tile +-1; M through one candidate, the candidate step +-1 and two steps + 1; the
# positives per context cycle through counts_for (B = 1 shapes take turns at its entries)
MEAN_SHAPES = [
    # k, k0, k1, kind, task, B, M, turn
    (0, 1, 1, VB, "r", REC_CTX + 1, REC_STEP + 1, 0),
    (1, 0, 1, ALS, "r", 1, 1, 1),
    (7, 1, 0, VB, "r", REC_CTX - 1, REC_STEP - 1, 2),
    (8, 1, 1, MCMC_DRAW, "c", REC_CTX + 1, REC_STEP, 3),
    (9, 0, 0, VB, "r", REC_TILE_B - 1, REC_STEP + 1, 4),
    (33, 1, 1, ALS, "r", REC_TILE_B + 1, 2 * REC_STEP + 1, 5),
    (64, 1, 1, VB_ONLINE, "r", REC_CTX - 1, 1, 0),
    (65, 0, 1, MCMC_DRAW, "c", 1, 2 * REC_STEP + 1, 5),            # one context, every candidate a positive
    (100, 1, 1, VB, "r", REC_TILE_B - 1, REC_STEP - 1, 1),
    (100, 1, 0, ALS, "r", 1, REC_STEP, 4),
]


@pytest.mark.parametrize("k,k0,k1,kind,task,B,M,turn", MEAN_SHAPES)
def test_mean_ranks_equal_the_oracle(tmp_path, k, k0, k1, kind, task, B, M, turn):
    m = make_model(tmp_path, kind, k, k0, k1, task=task)
    run_case(m, "mean", B, M, counts_for(M, turn), label="mean k=%d B=%d M=%d" % (k, B, M))
    m.close()


UCB_SHAPES = [
    # k, k0, k1, kind, B, M, turn, beta, noise, VBFM_UCB_CTX
    (0, 1, 1, VB, REC_CTX + 1, REC_STEP + 1, 0, 1.5, 0, "8"),
    (1, 0, 1, VB_ONLINE, 1, 1, 1, -1.5, 1, "16"),
    (7, 1, 0, VB, REC_CTX - 1, REC_STEP - 1, 2, 1.5, 1, "16"),
    (8, 1, 1, VB_ONLINE, REC_CTX + 1, REC_STEP, 3, -1.5, 0, "8"),
    (9, 0, 0, VB, REC_TILE_B - 1, REC_STEP + 1, 4, 1.5, 1, "8"),
    (33, 1, 1, VB, REC_TILE_B + 1, 2 * REC_STEP + 1, 5, -1.5, 0, "16"),
    (64, 1, 1, VB_ONLINE, REC_TILE_B + 1, 1, 0, 1.5, 0, "8"),
    (65, 0, 1, VB, 1, 2 * REC_STEP + 1, 5, -1.5, 1, "8"),
    (100, 1, 1, VB, REC_TILE_B - 1, REC_STEP - 1, 1, 1.5, 0, "16"),
    (100, 1, 0, VB_ONLINE, REC_CTX - 1, REC_STEP, 4, -1.5, 1, "8"),
]


@pytest.mark.parametrize("k,k0,k1,kind,B,M,turn,beta,noise,tile", UCB_SHAPES)
def test_ucb_ranks_equal_the_oracle(tmp_path, monkeypatch, k, k0, k1, kind, B, M, turn, beta, noise, tile):
    m = make_model(tmp_path, kind, k, k0, k1)
    monkeypatch.setenv("VBFM_UCB_CTX", tile)                   # the oracle's calls and the counting kernel alike
    run_case(m, "ucb", B, M, counts_for(M, turn), beta, bool(noise), label="ucb k=%d B=%d M=%d ctx=%s" % (k, B, M, tile))
    m.close()


CHAIN_SHAPES = [
    # k, k0, k1, S, task, B, M, turn, beta, noise
    (0, 1, 1, 1, "r", REC_CTX + 1, REC_STEP + 1, 0, 0.0, 0),
    (1, 0, 1, 3, "r", 1, 1, 1, 1.5, 1),
    (7, 1, 0, 3, "r", REC_CTX - 1, REC_STEP - 1, 2, -1.5, 0),
    (8, 1, 1, 1, "r", REC_CTX + 1, REC_STEP, 3, 1.5, 1),
    (9, 0, 0, 3, "c", REC_TILE_B - 1, REC_STEP + 1, 4, 0.0, 0),
    (33, 1, 1, 3, "r", REC_TILE_B + 1, 2 * REC_STEP + 1, 5, -1.5, 0),
    (64, 1, 1, 1, "r", REC_TILE_B - 1, 1, 0, 1.5, 0),
    (65, 0, 1, 3, "c", 1, 2 * REC_STEP + 1, 5, 1.5, 0),
    (100, 1, 1, 3, "r", REC_CTX - 1, REC_STEP - 1, 1, -1.5, 1),
]


@pytest.mark.parametrize("k,k0,k1,S,task,B,M,turn,beta,noise", CHAIN_SHAPES)
def test_chain_ranks_equal_the_oracle(tmp_path, k, k0, k1, S, task, B, M, turn, beta, noise):
    m = make_chain(tmp_path, k, k0, k1, S, task=task)[0]
    run_case(m, "chain", B, M, counts_for(M, turn), beta, bool(noise), label="chain k=%d S=%d B=%d M=%d" % (k, S, B, M))
    m.close()


# ---- 2. the defining property -------------------------------------------------------------------------
@pytest.mark.parametrize("ranking,beta,noise", [("mean", 0.0, False), ("ucb", -1.5, True), ("chain", 1.5, False)])
def test_rank_is_the_position_in_the_unbounded_recommend_list(tmp_path, ranking, beta, noise):
    m = model_for(tmp_path, ranking, 9)
    B, M = REC_CTX + 3, 100
    ctx, cand = contexts(B), candidates(M)
    excl = [np.arange(c % 5, M, 9, dtype=np.uint32) if c % 2 else np.zeros(0, dtype=np.uint32) for c in range(B)]
    pos = [np.setdiff1d(p, excl[c]).astype(np.uint32) for c, p in enumerate(positives_of(B, M, counts_for(M, 1)))]
    cs = make_set(m, ranking, cand)
    rank, key, ranked = m.rank_positives(ctx, cs, pos, exclude=excl, ranking=ranking, beta=beta, noise=noise)
    idx, rkey, count = recommend(m, ranking, ctx, cs, M, beta, noise, exclude=excl)
    assert np.array_equal(count, ranked)
    p = 0
    for c in range(B):
        for j in pos[c]:
            assert 0 <= rank[p] < count[c] and idx[c, rank[p]] == j and bits(rkey[c, rank[p]]) == bits(key[p]), (c, j)
            p += 1
    assert p == len(rank) and p > B
    # a shorter list: the positives of rank < topn are where they were, count is min(topn, ranked)
    idx5, rkey5, count5 = recommend(m, ranking, ctx, cs, 5, beta, noise, exclude=excl)
    assert np.array_equal(count5, np.minimum(5, ranked))
    assert np.array_equal(idx5, idx[:, :5])
    cs.close()
    m.close()


def test_one_draw_with_beta_zero_is_the_mean_ranking_of_that_draw(tmp_path):
    B, M = REC_CTX + 1, REC_STEP + 5
    ctx, cand = contexts(B), candidates(M)
    chain, path, _ = make_chain(tmp_path, 9, 1, 1, 1)
    one = draw_model(tmp_path, path, 0)
    pos = positives_of(B, M, counts_for(M, 1))
    cs_chain, cs_one = chain.candidates_chain(cand), one.candidates(cand)
    a = chain.rank_positives(ctx, cs_chain, pos, ranking="chain")
    b = one.rank_positives(ctx, cs_one, pos, ranking="mean")
    equal(a, b, "S = 1, beta = 0")
    for h in (cs_chain, cs_one, chain, one):
        h.close()


# ---- 3. exclusions -------------------------------------------------------------------------------------
@pytest.mark.parametrize("ranking,beta", [("mean", 0.0), ("ucb", 1.5), ("chain", -1.5)])
def test_excluded_candidates_are_taken_out_of_every_count(tmp_path, ranking, beta):
    m = model_for(tmp_path, ranking, 8)
    B, M = REC_CTX + 5, REC_STEP + 20
    # the lists of test_results_do_not_depend_on_chunks_slices_or_reuse, every fourth with a repeated index
    excl = [np.arange(c % 4, M, 7, dtype=np.uint32) if c % 3 else np.zeros(0, dtype=np.uint32) for c in range(B)]
    for c in range(1, B, 4):
        if len(excl[c]):
            excl[c] = np.sort(np.concatenate([excl[c], excl[c][2:4], excl[c][2:3]])).astype(np.uint32)
    got, want, K, pos = run_case(m, ranking, B, M, counts_for(M, 1), beta, exclude=excl, label="exclusions " + ranking)
    assert np.any(want[2] < M) and np.all(want[2][::3] == M)
    # one context, one positive: excluding a candidate that is before it lowers the rank by exactly one,
    # excluding one that is behind it changes nothing
    ctx, cand = contexts(B), candidates(M)
    cs = make_set(m, ranking, cand)
    c = 0
    order = np.lexsort((np.arange(M), -K[c]))                  # best first under the total order
    p, ahead, behind = int(order[M // 2]), int(order[3]), int(order[M - 2])
    one = [np.array([p], dtype=np.uint32)] + [np.zeros(0, dtype=np.uint32)] * (B - 1)
    with_x = lambda x: [np.array(x, dtype=np.uint32)] + [np.zeros(0, dtype=np.uint32)] * (B - 1)
    r0, k0, n0 = m.rank_positives(ctx, cs, one, ranking=ranking, beta=beta)
    r1, k1, n1 = m.rank_positives(ctx, cs, one, exclude=with_x([ahead]), ranking=ranking, beta=beta)
    r2, k2, n2 = m.rank_positives(ctx, cs, one, exclude=with_x([behind]), ranking=ranking, beta=beta)
    r3, k3, n3 = m.rank_positives(ctx, cs, one, exclude=with_x(sorted([ahead, ahead, behind])), ranking=ranking, beta=beta)
    assert r0[0] == M // 2 and n0[0] == M
    assert r1[0] == r0[0] - 1 and r2[0] == r0[0] and r3[0] == r0[0] - 1
    assert n1[0] == M - 1 and n2[0] == M - 1 and n3[0] == M - 2
    assert bits(k0[0]) == bits(k1[0]) == bits(k2[0]) == bits(k3[0]) == bits(K[c, p])
    cs.close()
    m.close()


# ---- 4. ties -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ranking,beta", [("mean", 0.0), ("ucb", 1.5), ("chain", 1.5)])
def test_duplicate_candidates_tie_and_the_lower_index_is_one_ahead(tmp_path, ranking, beta):
    m = model_for(tmp_path, ranking, 9)
    rp, f, v = candidates(40)
    lo, hi = 7, 31                                             # row hi becomes a copy of row lo
    rows = [(f[int(rp[j]):int(rp[j + 1])], v[int(rp[j]):int(rp[j + 1])]) for j in range(40)]
    rows[hi] = rows[lo]
    rp2 = np.zeros(41, dtype=np.uint64)
    np.cumsum([len(r[0]) for r in rows], out=rp2[1:])
    cand = (rp2, np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows]))
    B = 3
    ctx = contexts(B)
    cs = make_set(m, ranking, cand)
    both = [np.array([lo, hi], dtype=np.uint32)] * B
    rank, key, ranked = m.rank_positives(ctx, cs, both, ranking=ranking, beta=beta)
    assert np.all(ranked == 40)
    for c in range(B):
        assert rank[2 * c + 1] == rank[2 * c] + 1 and bits(key[2 * c]) == bits(key[2 * c + 1]), c
    equal((rank, key, ranked), oracle(key_matrix(m, ranking, ctx, cand, beta), both), "ties " + ranking)
    cs.close()
    m.close()


# ---- 5. pairs that are not finite ------------------------------------------------------------------------
@pytest.mark.parametrize("ranking,beta", [("mean", 0.0), ("ucb", 1.5), ("chain", 1.5)])
def test_nonfinite_candidates_are_in_no_count_and_have_no_rank(tmp_path, ranking, beta):
    B, M, a_inf, a_nan = 5, REC_STEP + 3, 77, 78
    D = D_SYNTH + 1                                            # ids 250 and 251 are in no context and in no other candidate
    ctx = contexts(B)
    rp, f, v = candidates(M)
    f = f.copy()
    f[int(rp[a_inf])] = D_SYNTH - 1
    f[int(rp[a_nan])] = D_SYNTH
    cand = (rp, f, v)

    def edit(p):
        w = p["mu_w"] if "mu_w" in p else p["w"]
        w[D_SYNTH - 1], w[D_SYNTH] = np.inf, np.nan

    def edit_draws(draws):
        draws[0]["w"][D_SYNTH - 1] = np.inf                    # one draw is enough: the chain's mean is not finite
        draws[2]["w"][D_SYNTH] = np.nan

    m = model_for(tmp_path, ranking, 7, D=D, edit=edit_draws if ranking == "chain" else edit)
    K = key_matrix(m, ranking, ctx, cand, beta)
    assert np.all(np.isnan(K[:, [a_inf, a_nan]])) and int(np.isnan(K).sum()) == 2 * B
    pos = [np.array(sorted({3, a_inf, a_nan, (11 * c) % M}), dtype=np.uint32) for c in range(B)]
    cs = make_set(m, ranking, cand)
    got = m.rank_positives(ctx, cs, pos, ranking=ranking, beta=beta)
    st = m.last_rank_stats
    want = oracle(K, pos)
    equal(got, want, "nonfinite " + ranking)
    assert st["nonfinite_pairs"] == 2 * B == want[3] and st["nonfinite_positives"] == 2 * B == want[4], st
    assert np.all(got[2] == M - 2)
    p = 0
    for c in range(B):
        for j in pos[c]:
            if j in (a_inf, a_nan):
                assert got[0][p] == -1 and np.isnan(got[1][p]), (c, j)
            else:
                assert got[0][p] >= 0 and np.isfinite(got[1][p]), (c, j)
            p += 1
    # excluded, they are taken out of nothing: they were in no count
    excl = [np.array([a_inf, a_nan], dtype=np.uint32)] * B
    fin = [np.setdiff1d(q, excl[0]).astype(np.uint32) for q in pos]
    equal(m.rank_positives(ctx, cs, fin, exclude=excl, ranking=ranking, beta=beta), oracle(K, fin, excl), "nonfinite, excluded")
    assert m.last_rank_stats["nonfinite_pairs"] == 2 * B
    cs.close()
    m.close()


# ---- 6. geometry independence ------------------------------------------------------------------------------
@pytest.mark.parametrize("ranking,beta", [("mean", 0.0), ("ucb", -1.5), ("chain", 1.5)])
def test_results_do_not_depend_on_slices_chunks_tile_or_reuse(tmp_path, monkeypatch, ranking, beta):
    m = model_for(tmp_path, ranking, 33)
    B, M = REC_TILE_B + 5, 3 * REC_STEP + 9
    ctx, cand = contexts(B), candidates(M)
    excl = [np.arange(c % 4, M, 7, dtype=np.uint32) if c % 3 else np.zeros(0, dtype=np.uint32) for c in range(B)]
    pos = [np.setdiff1d(p, excl[c]).astype(np.uint32) for c, p in enumerate(positives_of(B, M, counts_for(M, 2)))]
    monkeypatch.delenv("VBFM_REC_SLICES", raising=False)
    monkeypatch.delenv("VBFM_UCB_CTX", raising=False)
    cs = make_set(m, ranking, cand)
    call = lambda **kw: m.rank_positives(ctx, cs, pos, exclude=excl, ranking=ranking, beta=beta, **kw)
    base = call()
    assert m.last_rank_stats["n_chunks"] == 1 and m.last_rank_stats["passes"] > 2
    equal(base, oracle(key_matrix(m, ranking, ctx, cand, beta), pos, excl), "geometry base " + ranking)
    equal(call(), base, "the candidate set reused")
    row_bytes = 8 + F * 8
    for chunk_bytes, chunks in ((1 << 20, 1), (8 + 23 * row_bytes, 3), (1, B)):
        equal(call(chunk_bytes=chunk_bytes), base, "chunk_bytes=%d" % chunk_bytes)
        if ranking != "chain":                                 # (a chain's chunks also hold its prepared sums, 8 rows at least)
            assert m.last_rank_stats["n_chunks"] == chunks, (chunk_bytes, m.last_rank_stats)
        else:
            assert (m.last_rank_stats["n_chunks"] > 1) == (chunks > 1), (chunk_bytes, m.last_rank_stats)
    for slices in ("1", "3", "64"):                            # read at every call
        monkeypatch.setenv("VBFM_REC_SLICES", slices)
        equal(call(), base, "slices=" + slices)
        equal(call(chunk_bytes=8 + 23 * row_bytes), base, "3 chunks, slices=" + slices)
    if ranking == "ucb":
        for tile in ("8", "16"):
            monkeypatch.setenv("VBFM_UCB_CTX", tile)
            equal(call(), base, "tile=" + tile)
    cs.close()
    m.close()


# ---- 7. refusals: the message names the offender, nothing is written ---------------------------------------------
def raw_call(m, cs, ctx, pos_ptr, pos_idx, excl_ptr=None, excl_idx=None, ranking=0, unknown_ids=0, beta=0.0, noise=0,
             null=()):
    """vbfm_rank_positives through ctypes with sentinel-filled outputs: (rc, message, outputs untouched)."""
    L = vbfm.lib()
    rows, _keep = vbfm.Model._rows(ctx)
    B = rows.num_rows
    u64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint64)
    u32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint32)
    pp, pi, xp, xi = u64(pos_ptr), u32(pos_idx), u64(excl_ptr), u32(excl_idx)
    n = 64
    key, rank, ranked = np.full(n, 7.5), np.full(n, 12345, dtype=np.int64), np.full(max(B, n), 54321, dtype=np.uint32)
    o = vbfm.RankPositivesOpts(ranking, unknown_ids, 0, beta, noise)
    st = vbfm.RankPositivesStats()
    P = vbfm._ptr
    rc = L.vbfm_rank_positives(m._m, None if "cs" in null else cs._c, None if "contexts" in null else C.byref(rows),
                               P(xp, vbfm.P_u64), P(xi, vbfm.P_u32), None if "pos_ptr" in null else P(pp, vbfm.P_u64),
                               P(pi, vbfm.P_u32), None if "opts" in null else C.byref(o),
                               None if "key" in null else P(key, vbfm.P_f64),
                               None if "rank" in null else rank.ctypes.data_as(C.POINTER(C.c_int64)),
                               None if "ranked" in null else P(ranked, vbfm.P_u32), C.byref(st))
    msg = L.vbfm_model_last_error(m._m)
    untouched = bool(np.all(key == 7.5) and np.all(rank == 12345) and np.all(ranked == 54321))
    return rc, (msg.decode() if msg else ""), untouched


def test_refusals(tmp_path):
    B, M = 4, 20
    ctx, cand = contexts(B), candidates(M)
    dirs = {}
    for name in ("vb", "als", "other", "big", "chain", "chain_c"):
        (tmp_path / name).mkdir()
        dirs[name] = tmp_path / name
    vb, als = make_model(dirs["vb"], VB, 8, 1, 1), make_model(dirs["als"], ALS, 8, 1, 1)
    other = make_model(dirs["other"], VB, 8, 1, 1)
    big = make_model(dirs["big"], ALS, 257, 1, 1, D=8)
    chain = make_chain(dirs["chain"], 8, 1, 1, 2)[0]
    chain_c = make_chain(dirs["chain_c"], 8, 1, 1, 2, task="c")[0]
    cs_plain, cs_var, cs_als = vb.candidates(cand), vb.candidates(cand, variance=True), als.candidates(cand)
    cs_chain, cs_chain_c = chain.candidates_chain(cand), chain_c.candidates_chain(cand)
    ptr, idx = [0, 1, 1, 3, 4], [5, 2, 9, 0]
    xptr, xidx = [0, 0, 2, 3, 3], [4, 4, 9]                     # context 2 excludes its positive 9
    MEAN, UCB, CHAIN = 0, 1, 2
    who = "vbfm_rank_positives: "
    cases = [
        # model, set, keyword arguments of raw_call, message
        (vb, cs_plain, dict(null=("cs",)), "null argument"),
        (vb, cs_plain, dict(null=("contexts",)), "null argument"),
        (vb, cs_plain, dict(null=("opts",)), "null argument"),
        (vb, cs_plain, dict(null=("pos_ptr",)), "null argument"),
        (vb, cs_plain, dict(null=("key",)), "null result array"),
        (vb, cs_plain, dict(null=("rank",)), "null result array"),
        (vb, cs_plain, dict(null=("ranked",)), "null result array"),
        (vb, cs_plain, dict(ranking=3), "ranking = 3 is none of"),
        (vb, cs_plain, dict(pos_ptr=[1, 1, 1, 3, 4]), "pos_ptr does not start at 0"),
        (vb, cs_plain, dict(pos_ptr=[0, 2, 1, 3, 4]), "pos_ptr is not monotone at context row 1"),
        (vb, cs_plain, dict(pos_idx=[5, 2, M, 0]), "positive list of context row 2 holds candidate index %d, but the candidate set has %d rows" % (M, M)),
        (vb, cs_plain, dict(pos_idx=[5, 9, 2, 0]), "positive list of context row 2 is not strictly ascending"),
        (vb, cs_plain, dict(pos_idx=[5, 2, 2, 0]), "positive list of context row 2 is not strictly ascending"),
        (vb, cs_plain, dict(excl_ptr=xptr, excl_idx=xidx), "candidate index 9 is a positive of context row 2 and on its exclusion list"),
        (vb, cs_plain, dict(excl_ptr=[0, 0, 2, 3, 3], excl_idx=[4, 3, 7]), "exclusion list of context row 1 is not sorted"),
        (vb, cs_plain, dict(unknown_ids=2), "unknown_ids is 0 (refuse) or 1 (skip)"),
        (vb, cs_plain, dict(beta=1.5), "with VBFM_RANKING_MEAN"),
        (vb, cs_plain, dict(noise=1), "with VBFM_RANKING_MEAN"),
        (vb, cs_var, dict(ranking=UCB, beta=float("nan")), "is not a finite number"),
        (vb, cs_var, dict(ranking=UCB, beta=float("inf")), "is not a finite number"),
        (vb, cs_var, dict(ranking=UCB, noise=2), "noise is 0 or 1"),
        (vb, cs_plain, dict(ranking=UCB, beta=1.0), "holds no variance sums"),
        (als, cs_als, dict(ranking=UCB, beta=1.0), "VBFM_MODEL_ALS holds no posterior variances"),
        (other, cs_plain, dict(), "made from another model"),
        (other, cs_var, dict(ranking=UCB, beta=1.0), "made from another model"),
        (big, cs_als, dict(), "num_factor = 257 is beyond the limit of 256"),
        (chain, cs_chain, dict(), "a chain of draws (VBFM_MODEL_MCMC_CHAIN) is scored, not ranked"),
        (chain, cs_chain, dict(ranking=UCB, beta=1.0), "a chain of draws (VBFM_MODEL_MCMC_CHAIN) is scored, not ranked"),
        (vb, cs_plain, dict(ranking=CHAIN), "VBFM_MODEL_VB holds one set of parameters, not a chain of draws"),
        (chain_c, cs_chain_c, dict(ranking=CHAIN, beta=1.0, noise=1), "a model of task c has no noise precision"),
        (chain, cs_chain_c, dict(ranking=CHAIN), "made from another model"),
        (chain, cs_chain, dict(ranking=CHAIN, beta=float("nan")), "is not a finite number"),
    ]
    for m, cs, kw, message in cases:
        args = dict(pos_ptr=ptr, pos_idx=idx)
        args.update(kw)
        rc, msg, untouched = raw_call(m, cs, ctx, **args)
        assert rc != 0 and message in msg and untouched, (kw, message, msg)
        if "null" not in message:
            assert msg.startswith(who), msg
    # a set of vbfm_candidates_create handed to a chain model's call, and a chain's set to vbfm_recommend's ranking
    rc, msg, untouched = raw_call(vb, cs_chain, ctx, ptr, idx)
    assert rc != 0 and untouched and "vbfm_candidates_create_chain); vbfm_recommend_chain ranks it" in msg, msg
    rc, msg, untouched = raw_call(chain, cs_plain, ctx, ptr, idx, ranking=CHAIN)
    assert rc != 0 and untouched and "use vbfm_candidates_create_chain" in msg, msg
    # the well-formed call goes through, through the same helper
    rc, msg, untouched = raw_call(vb, cs_plain, ctx, ptr, idx, excl_ptr=[0, 0, 2, 3, 3], excl_idx=[4, 4, 7])
    assert rc == 0 and not untouched, msg
    with pytest.raises(vbfm.VbfmError, match="ranking is one of"):
        vb.rank_positives(ctx, cs_plain, (np.array(ptr), np.array(idx)), ranking="best")
    for h in (cs_plain, cs_var, cs_als, cs_chain, cs_chain_c, vb, als, other, big, chain, chain_c):
        h.close()


# ---- 8. the CLI ----------------------------------------------------------------------------------------------------
def eval_line(pos, rank, ranked, at):
    """The launcher's #Eval line from vbfm.ranking_metrics, at its 6 significant digits."""
    mt = vbfm.ranking_metrics(pos, rank, ranked, at=at)
    with_pos = [c for c, p in enumerate(pos) if len(p)]
    ranked_sum = 0.0
    for c in with_pos:
        ranked_sum += float(ranked[c])
    g = lambda x: "%.6g" % x
    line = "#Eval contexts=%d positives=%d ranked_mean=%s" % (mt["contexts"], mt["positives"], g(ranked_sum / len(with_pos)))
    for N in at:
        line += " HR@%d=%s NDCG@%d=%s recall@%d=%s" % (N, g(mt["hr@%d" % N]), N, g(mt["ndcg@%d" % N]), N, g(mt["recall@%d" % N]))
    return line + " MRR=%s AUC=%s" % (g(mt["mrr"]), g(mt["auc"]))


@pytest.mark.parametrize("ranking", ["mean", "ucb", "chain"])
def test_cli_positives(tmp_path, ranking):
    d = os.path.join(GOLDEN, "tiny")
    tr, te = os.path.join(d, "train.libfm"), os.path.join(d, "test.libfm")
    items, users = vbfm.DataSubset.load(tr), vbfm.DataSubset.load(te)
    D = vbfm.num_all_attribute(items, users)
    m = model_for(tmp_path, ranking, 3, D=D, mn=float(items.min_target), mx=float(items.max_target))
    mfile = [str(p) for p in tmp_path.iterdir() if str(p).endswith(".vbfm")][0]
    B, M = users.num_cases, items.num_cases
    rng = np.random.default_rng(9)
    excl = [rng.permutation(M)[:rng.integers(0, 4)] for _ in range(B)]
    held = [np.setdiff1d(rng.permutation(M)[:rng.integers(0, 4)], excl[c]) for c in range(B)]
    held[0] = np.array([x % M for x in (2, 0, 2, 1) if x % M not in excl[0]], dtype=np.int64)   # any order, with a duplicate
    held[B - 1] = np.zeros(0, dtype=np.int64)                                  # an empty line
    for name, lists in (("ex", excl), ("held", held)):
        with open(tmp_path / name, "w") as fh:
            for e in lists:
                fh.write(" ".join(str(int(x)) for x in e) + "\n")
    at = (1, 3, 10)
    flags = {"mean": [], "ucb": ["-ucb", "-1.5", "-ucb_noise", "1"], "chain": ["-ucb", "1.5"]}[ranking]
    beta, noise = {"mean": (0.0, False), "ucb": (-1.5, True), "chain": (1.5, False)}[ranking]
    r = subprocess.run([CLI, "-load_model", mfile, "-test", te, "-candidates", tr, "-positives", "held", "-exclude", "ex",
                        "-eval_at", "1,3,10,3", "-out", "ranks"] + flags, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    cs = make_set(m, ranking, items)
    pos = [np.unique(e).astype(np.uint32) for e in held]
    rank, key, ranked = m.rank_positives(users, cs, pos, exclude=[np.unique(e).astype(np.uint32) for e in excl],
                                         ranking=ranking, beta=beta, noise=noise)
    assert len(rank) > 0 and np.all(rank >= 0)
    want, p = [], 0
    for c in range(B):
        want.append(" ".join("%d:%d:%.17g" % (pos[c][i], rank[p + i], key[p + i]) for i in range(len(pos[c]))))
        p += len(pos[c])
    got = open(tmp_path / "ranks").read().split("\n")
    assert got[-1] == "" and got[:-1] == want
    lines = [ln for ln in r.stdout.split("\n") if ln.startswith("#Eval")]
    assert lines == [eval_line(pos, rank, ranked, at)], (lines, r.stdout[-1000:])
    # -out is optional: the line alone
    os.remove(tmp_path / "ranks")
    r = subprocess.run([CLI, "-load_model", mfile, "-test", te, "-candidates", tr, "-positives", "held", "-exclude", "ex"] + flags,
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not os.path.exists(tmp_path / "ranks"), r.stderr[-2000:]
    assert [ln for ln in r.stdout.split("\n") if ln.startswith("#Eval")] == [eval_line(pos, rank, ranked, (5, 10, 20))]
    cs.close()
    m.close()

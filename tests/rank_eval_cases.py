"""What tests/test_rank_eval_gpu.py and tests/test_rank_eval_cpu.py share: the oracle of
Model.rank_positives (include/vbfm.h "ranking held-out candidates") and a brute-force restatement of
vbfm.ranking_metrics. It builds on tests/recommend_cases.py and tests/recommend_chain_cases.py.

The oracle needs no tolerance. The full key matrix [B, M] of a ranking comes from that ranking's own
recommend call (clip=False, topn=128) over candidate subsets of at most 128 rows: a pair's bits depend
on its two rows only (pair_bits_depend_on_the_rows_only asserts that), every pair that is ok is
returned because topn covers the subset, and a pair that is not returned is not ok (NaN in the
matrix). Ranks and `ranked` are then counted in numpy with the total order -- larger key first, equal
keys by smaller index -- and compared for equality. The assertions are in the test files."""
import numpy as np

from recommend_cases import bits

EVAL_POS = 8                      # csrc/vbfm_recommend.hip: positives of a context a wave holds per pass
SUB = 128                         # vbfm.REC_MAX_TOPN: the oracle's candidate subsets
RANKINGS = ("mean", "ucb", "chain")


def rows_subset(rows, sel):
    """The rows `sel` (indices) of a (row_ptr, feat, val) triple."""
    rp, f, v = rows
    rp = rp.astype(np.int64)
    lens = [rp[j + 1] - rp[j] for j in sel]
    out = np.zeros(len(sel) + 1, dtype=np.uint64)
    np.cumsum(lens, out=out[1:])
    cat = lambda a: (np.concatenate([a[rp[j]:rp[j + 1]] for j in sel]) if len(sel) else a[:0])
    return out, cat(f), cat(v)


def make_set(m, ranking, cand):
    if ranking == "chain":
        return m.candidates_chain(cand)
    return m.candidates(cand, variance=(ranking == "ucb"))


def recommend(m, ranking, ctx, cs, topn, beta=0.0, noise=False, exclude=None):
    """(idx, key, count) of the ranking's own recommend call, clip=False: key is what it ranked on."""
    if ranking == "mean":
        idx, score, count = m.recommend(ctx, cs, topn, exclude=exclude, clip=False)
        return idx, score, count
    call = m.recommend_ucb if ranking == "ucb" else m.recommend_chain
    idx, key, _score, _var, count = call(ctx, cs, topn, beta=beta, noise=noise, exclude=exclude, clip=False)
    return idx, key, count


def subset_keys(m, ranking, ctx, cand, sel, beta=0.0, noise=False):
    """keys [B, len(sel)] of the candidates `sel` ranked as a set of their own; NaN: the pair is not ok."""
    B = len(ctx[0]) - 1
    out = np.full((B, len(sel)), np.nan)
    if not len(sel) or not B:
        return out
    assert len(sel) <= SUB
    cs = make_set(m, ranking, rows_subset(cand, sel))
    idx, key, count = recommend(m, ranking, ctx, cs, SUB, beta, noise)
    cs.close()
    for c in range(B):
        n = int(count[c])
        out[c, idx[c, :n].astype(np.int64)] = key[c, :n]
    return out


def key_matrix(m, ranking, ctx, cand, beta=0.0, noise=False):
    """The full key matrix [B, M] from subsets of at most SUB consecutive candidate rows."""
    M = len(cand[0]) - 1
    parts = [subset_keys(m, ranking, ctx, cand, np.arange(a, min(a + SUB, M)), beta, noise) for a in range(0, M, SUB)]
    return np.concatenate(parts, axis=1) if parts else np.zeros((len(ctx[0]) - 1, 0))


def pair_bits_depend_on_the_rows_only(m, ranking, ctx, cand, beta=0.0, noise=False):
    """On a candidate set of at most SUB rows: the full set and two subsets agree bit for bit."""
    M = len(cand[0]) - 1
    assert 2 <= M <= SUB
    full = subset_keys(m, ranking, ctx, cand, np.arange(M), beta, noise)
    for sel in (np.arange(0, M, 2), np.arange(M // 3, M)[::-1]):
        part = subset_keys(m, ranking, ctx, cand, sel, beta, noise)
        assert np.array_equal(bits(part), bits(full[:, sel])), (ranking, sel[:4])
    return full


def before(K, j, kp, p):
    """rec_better(K[j], j, kp, p) for the index array j."""
    return (K[j] > kp) | ((K[j] == kp) & (j < p))


def oracle(K, positives, exclude=None):
    """(rank int64 [P], key [P], ranked uint32 [B], nonfinite pairs, nonfinite positives) of a key matrix."""
    B, M = K.shape
    rank, key, ranked = [], [], np.zeros(B, dtype=np.uint32)
    for c in range(B):
        ok = ~np.isnan(K[c])
        if exclude is not None and len(exclude[c]):
            ok[np.asarray(exclude[c], dtype=np.int64)] = False
        j = np.nonzero(ok)[0]
        ranked[c] = len(j)
        for p in np.asarray(positives[c], dtype=np.int64):
            kp = K[c, p]
            key.append(kp)
            rank.append(-1 if np.isnan(kp) else int(np.count_nonzero(before(K[c], j, kp, p))))
    rank = np.asarray(rank, dtype=np.int64)
    return rank, np.asarray(key, dtype=np.float64), ranked, int(np.isnan(K).sum()), int((rank < 0).sum())


def positives_of(B, M, counts, seed=11):
    """One strictly ascending list per context, context c with min(counts[c % len(counts)], M) positives."""
    rng = np.random.default_rng(seed)
    return [np.sort(rng.permutation(M)[:min(counts[c % len(counts)], M)]).astype(np.uint32) for c in range(B)]


def equal(got, want, label=""):
    """rank, key bits and ranked of Model.rank_positives against the oracle's first three results."""
    assert got[0].dtype == np.int64 and got[2].dtype == np.uint32, label
    assert np.array_equal(got[0], want[0]), (label, "rank", got[0][:16], want[0][:16])
    assert np.array_equal(bits(got[1]), bits(want[1])), (label, "key")
    assert np.array_equal(got[2], want[2]), (label, "ranked", got[2][:16], want[2][:16])


def brute_metrics(positives, rank, ranked, at):
    """vbfm.ranking_metrics restated from the definitions, context by context, with python floats."""
    import math
    out = {}
    rows, p0 = [], 0
    for c, pos in enumerate(positives):
        r = [int(x) for x in rank[p0:p0 + len(pos)]]
        p0 += len(pos)
        if len(pos):
            rows.append((len(pos), sorted(x for x in r if x >= 0), int(ranked[c])))
    nc = len(rows)
    for N in at:
        out["hr@%d" % N] = sum(1.0 for n, r, _ in rows if any(x < N for x in r)) / nc
        out["recall@%d" % N] = sum(sum(1 for x in r if x < N) / n for n, r, _ in rows) / nc
        out["ndcg@%d" % N] = sum(sum(1.0 / math.log2(x + 2) for x in r if x < N) /
                                 sum(1.0 / math.log2(i + 2) for i in range(min(n, N))) for n, r, _ in rows) / nc
    out["mrr"] = sum(1.0 / (r[0] + 1) if r else 0.0 for _, r, _ in rows) / nc
    aucs = []
    for _, r, rk in rows:
        nn = rk - len(r)
        if r and nn > 0:
            # the share of (positive, negative) pairs the positive wins: a negative is before positive i when
            # it is one of the r_(i) - (i - 1) non-positives ahead of it
            aucs.append(sum(nn - (x - i) for i, x in enumerate(r)) / (len(r) * nn))
    out["auc"] = sum(aucs) / len(aucs) if aucs else float("nan")
    out["auc_contexts"] = len(aucs)
    out["contexts"] = nc
    return out

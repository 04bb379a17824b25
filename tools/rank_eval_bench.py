#!/usr/bin/env python3
"""Held-out evaluation throughput on one MI355X: the counting kernel of vbfm_rank_positives beside the
pair kernel of the ranking's own top-N call on the same inputs. All times are
device-event times the library reports.

--contexts (65,536) rows of 39 fields x 25,000 ids (tests/synth.py), x != 1, in host memory, against
--candidates (100,000) single-entry rows over ids of their own; every context has one positive and 20
exclusions (distinct from it). Per k in --k (8 20 50 100), for the rankings mean (vbfm_recommend) and
ucb (vbfm_recommend_ucb, beta 1.5), and for one chain shape (--chain-k 20, --chain-draws 16,
vbfm_recommend_chain, beta 1.5):
    eval       Model.rank_positives; ms_prepare / ms_keys / ms_count / ms_finish of the call;
    topn       the ranking's recommend call at topn = 10 with the same exclusions; ms_pairs.
Both alternate in one process, --rounds (5) rounds after a warm-up round. Reported: every time, the
medians, each side's spread (max - min over median) and ratio = median ms_count / median ms_pairs.
Same results: for the first --check-contexts (64) contexts, a positive of rank < 10 is where the top-N
call put it, with the same key bits.

Writes one JSON document to --out and prints it. Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scalable-variational-bayesian-factorization-machine_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

F, S = 39, 25000
TOPN, BETA, N_EXCL = 10, 1.5, 20
EVAL_PHASES = ("ms_prepare", "ms_keys", "ms_count", "ms_finish")


def median(xs):
    return float(np.median(np.asarray(xs, dtype=np.float64)))


def spread(xs):
    return (max(xs) - min(xs)) / median(xs)


def vb_model(vbfm, k, D):
    fml = vbfm.FMLearnVB(1, 1, k, D, min_target=1.0, max_target=5.0, layout="column")
    fml.init_device(11)
    m = vbfm.Model.from_learner(fml)
    fml.close()
    return m


def chain_model(vbfm, k, D, draws):
    def learner(seed):
        fml = vbfm.FMLearnMCMC(1, 1, k, D, min_target=1.0, max_target=5.0, method="mcmc", layout="column")
        fml.init(seed, 0.1, rng=vbfm.RNG_DEVICE)
        return fml
    first = learner(100)
    ch = first.chain(draws)
    ch.add(first)
    for s in range(1, draws):
        fml = learner(100 + s)
        ch.add(fml)
        fml.close()
    model = ch.model()
    ch.close()
    first.close()
    return model


def lists(B, M, seed):
    """(positives, exclusions) as (ptr, idx) pairs: one positive and N_EXCL other candidates per context."""
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, M, size=B).astype(np.uint32)
    # N_EXCL offsets in 1 .. M - 1 from the positive: never the positive itself (a rare repeat counts once)
    off = rng.integers(1, M, size=(B, N_EXCL))
    excl = np.sort((pos[:, None].astype(np.int64) + off) % M, axis=1).astype(np.uint32)
    return ((np.arange(B + 1, dtype=np.uint64), pos),
            (np.arange(B + 1, dtype=np.uint64) * np.uint64(N_EXCL), excl.ravel()))


def measure(m, cs, ranking, ctx, pos, excl, a):
    beta = 0.0 if ranking == "mean" else BETA
    ev = {key: [] for key in EVAL_PHASES}
    pairs, check = [], None
    for r in range(a.rounds + 1):                      # round 0 warms every kernel and buffer up
        rank, key, ranked = m.rank_positives(ctx, cs, pos, exclude=excl, ranking=ranking, beta=beta)
        st = dict(m.last_rank_stats)
        if ranking == "mean":
            idx, rkey, count = m.recommend(ctx, cs, TOPN, exclude=excl, clip=False)
        elif ranking == "ucb":
            idx, rkey, _, _, count = m.recommend_ucb(ctx, cs, TOPN, beta, exclude=excl, clip=False)
        else:
            idx, rkey, _, _, count = m.recommend_chain(ctx, cs, TOPN, beta, exclude=excl, clip=False)
        if r:
            for k in EVAL_PHASES:
                ev[k].append(st[k])
            pairs.append(m.last_recommend_stats["ms_pairs"])
        else:
            n, hits, same = a.check_contexts, 0, True
            for c in range(n):
                if 0 <= rank[c] < TOPN:
                    hits += 1
                    same &= bool(idx[c, rank[c]] == pos[1][c] and rkey[c, rank[c]].view(np.uint64) == key[c:c + 1].view(np.uint64)[0])
            same &= bool(np.array_equal(count[:n], np.minimum(TOPN, ranked[:n])))
            check = {"contexts": n, "positives_in_the_top_n": hits, "same_place_and_bits": same,
                     "passes": st["passes"], "n_chunks": st["n_chunks"], "mean_rank": float(np.mean(rank))}
    med = {k: median(v) for k, v in ev.items()}
    return {"eval": {**ev, "median_ms": med, "spread_count": spread(ev["ms_count"])},
            "topn": {"topn": TOPN, "ms_pairs": pairs, "median_ms": median(pairs), "spread_pairs": spread(pairs)},
            "ratio_count_over_pairs": med["ms_count"] / median(pairs), "check": check}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--contexts", type=int, default=65536)
    ap.add_argument("--candidates", type=int, default=100_000)
    ap.add_argument("--k", type=int, nargs="+", default=[8, 20, 50, 100])
    ap.add_argument("--chain-k", type=int, default=20)
    ap.add_argument("--chain-draws", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--check-contexts", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_eval", "rank_eval_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rank_eval_bench.py needs a GPU")
    torch.cuda.init()
    import synth
    import vbfm
    B, M = a.contexts, a.candidates
    D = F * S + M + 1
    rp, f, v, _ = synth.generate(B, F, S, 301, 1)
    ctx = (rp, f, v)
    cand = (np.arange(M + 1, dtype=np.uint64), np.arange(F * S, F * S + M, dtype=np.uint32), np.ones(M, dtype=np.float32))
    pos, excl = lists(B, M, 17)
    shapes = []
    for k in a.k:
        m = vb_model(vbfm, k, D)
        cs = m.candidates(cand, variance=True)         # serves both rankings, with the same bits
        for ranking in ("mean", "ucb"):
            doc = {"ranking": ranking, "k": k, "draws": 1, "contexts": B, "candidates": M, "pairs": B * M,
                   **measure(m, cs, ranking, ctx, pos, excl, a)}
            shapes.append(doc)
            print(json.dumps(doc), flush=True)
        cs.close()
        m.close()
    if a.chain_draws:
        m = chain_model(vbfm, a.chain_k, D, a.chain_draws)
        cs = m.candidates_chain(cand)
        doc = {"ranking": "chain", "k": a.chain_k, "draws": a.chain_draws, "contexts": B, "candidates": M, "pairs": B * M,
               **measure(m, cs, "chain", ctx, pos, excl, a)}
        shapes.append(doc)
        print(json.dumps(doc), flush=True)
        cs.close()
        m.close()
    doc = {"device": torch.cuda.get_device_name(0), "positives_per_context": 1, "exclusions_per_context": N_EXCL,
           "rounds": a.rounds, "slices_override": os.environ.get("VBFM_REC_SLICES"),
           "tile_override": os.environ.get("VBFM_UCB_CTX"), "shapes": shapes}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()

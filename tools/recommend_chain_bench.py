#!/usr/bin/env python3
"""Top-N from a chain of draws on one MI355X: vbfm_recommend_chain against (1) the parent's only way to
the same answer -- every (context, candidate) pair expanded into one row and pushed through vbfm_score
of the chain model with var -- and (2) its yardstick, S calls of vbfm_recommend on one-draw models,
which do the same FMAs and no moments (shapes and conventions of
tools/recommend_ucb_bench.py, §14). All times are device-event times the library reports.

Throughput regime. C3's feature space, 40 fields x 25,000 ids; --contexts rows of the first 39 fields,
the 25,000 ids of the last field as single-entry candidates. The draws are S learners'
device-initialised parameters (as tools/chain_bench.py makes them). Per k in --k, S in --draws and topn
in --topn:
    chain      vbfm_recommend_chain (beta --beta, noise 1);
    one_draw   vbfm_recommend of the MCMC_DRAW model of draw 0 on the same inputs; the yardstick is S
               times its ms_pairs (every draw costs the same: the shapes are equal);
    baseline   --baseline-contexts contexts expanded to rows of 40 entries through vbfm_score(var) of
               the chain model, order = group, kernel time only, scaled per pair.
    All alternate in one process, --rounds (3) rounds after a warm-up round; medians and spreads
    ((max - min) / median). check: the first --check-contexts contexts' top-N recomputed from the
    baseline's means and spreads.
Serving regime. B = 1 against --serve-m (1e6) single-entry candidates, k = --serve-k (20), S =
--serve-draws (8), topn 10: ms_pairs and the bytes/s of streaming the set's Q (S * M * k * 8) against
the guides' achievable HBM rate.

Writes one JSON document to --out and prints it. Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from recommend_bench import F, HBM_ACHIEVABLE, S as IDS, expand, median   # noqa: E402  (it puts the package and tests on sys.path)

PHASES = ("ms_prepare", "ms_pairs", "ms_merge")
MN, MX = 1.0, 5.0


def spread(xs):
    return (max(xs) - min(xs)) / median(xs)


def timed(store, stats):
    for key in PHASES:
        store[key].append(stats[key])


def summary(store):
    med = {key: median(vals) for key, vals in store.items()}
    return {**store, "median_ms": med, "total_ms": sum(med.values()), "spread_pairs": spread(store["ms_pairs"])}


def chain_and_draw(vbfm, k, D, S):
    """(chain model of S device-initialised draws, the MCMC_DRAW model of draw 0, mean of 1 / alpha)."""
    def learner(seed):
        fml = vbfm.FMLearnMCMC(1, 1, k, D, min_target=MN, max_target=MX, method="mcmc", layout="column")
        fml.init(seed, 0.1, rng=vbfm.RNG_DEVICE)
        return fml
    first = learner(100)
    ch = first.chain(S)
    ch.add(first)
    one = vbfm.Model.from_learner(first)
    for s in range(1, S):
        fml = learner(100 + s)
        ch.add(fml)
        fml.close()
    model = ch.model()
    ch.close()
    first.close()
    na = float(np.mean(1.0 / model.draw_scalars()[1]))
    return model, one, na


def throughput(vbfm, synth, a):
    D = F * IDS + 1
    B = a.contexts
    rp, f, v, _ = synth.generate(B, F - 1, IDS, 301, 1)
    ctx = (rp, f, v)
    cand_ids = np.arange((F - 1) * IDS, F * IDS, dtype=np.uint32)
    M = len(cand_ids)
    cand = (np.arange(M + 1, dtype=np.uint64), cand_ids, np.ones(M, dtype=np.float32))
    nb = a.baseline_contexts
    base_rows = expand(ctx, cand_ids, nb)
    out = []
    for k in a.k:
        for S in a.draws:
            m, one, na = chain_and_draw(vbfm, k, D, S)
            cs, cs1 = m.candidates_chain(cand), one.candidates(cand)
            new = lambda: {key: [] for key in PHASES}
            base_ms = []
            rec = {t: {"chain": new(), "one_draw": new()} for t in a.topn}
            check = None
            for r in range(a.rounds + 1):                # round 0 warms every kernel and buffer up
                mean, var = m.score(base_rows, variance=True, order="group", clip=False)
                if r:
                    base_ms.append(m.last_stats["ms_kernel"])
                for t in a.topn:
                    one.recommend(ctx, cs1, t, clip=False)
                    if r:
                        timed(rec[t]["one_draw"], one.last_recommend_stats)
                    res = m.recommend_chain(ctx, cs, t, a.beta, noise=True, clip=False)
                    if r:
                        timed(rec[t]["chain"], m.last_recommend_stats)
                    if r == 0 and t == a.topn[0]:        # the same answer as the baseline's
                        n = min(a.check_contexts, nb)
                        ref_m, ref_v = mean.reshape(nb, M)[:n], var.reshape(nb, M)[:n]
                        ref_k = ref_m + a.beta * np.sqrt(ref_v + na)
                        top = np.sort(ref_k, axis=1)[:, ::-1][:, :t]
                        idx = res[0][:n].astype(np.int64)
                        rel = lambda x, y: float(np.max(np.abs(x - y) / np.maximum(1.0, np.abs(y))))
                        check = {"contexts": n, "topn": t, "beta": a.beta, "noise": 1,
                                 "rel_key_diff": rel(res[1][:n], top),
                                 "rel_diff_of_picked": rel(np.take_along_axis(ref_k, idx, axis=1), top),
                                 "rel_score_diff": rel(res[2][:n], np.take_along_axis(ref_m, idx, axis=1)),
                                 "abs_var_diff": float(np.max(np.abs(res[3][:n] - np.take_along_axis(ref_v, idx, axis=1))))}
            b = median(base_ms)
            base_pairs = nb * M / (b * 1e-3)
            doc = {"k": k, "draws": S, "contexts": B, "candidates": M, "pairs": B * M,
                   "chain_set_bytes": S * (k + 1) * ((M + 127) // 128 * 128) * 8,
                   "baseline": {"rows": nb * M, "ms_kernel": base_ms, "median_ms": b, "spread": spread(base_ms),
                                "pairs_per_s": base_pairs},
                   "check": check, "topn": []}
            for t in a.topn:
                c, o = summary(rec[t]["chain"]), summary(rec[t]["one_draw"])
                c["pairs_per_s"] = B * M / (c["total_ms"] * 1e-3)
                c["speedup_vs_baseline"] = c["pairs_per_s"] / base_pairs
                c["faster_by_more_than_spread"] = c["pairs_per_s"] > base_pairs * (1 + doc["baseline"]["spread"])
                c["pair_kernel_fma_per_s"] = float(B) * M * k * S / (c["median_ms"]["ms_pairs"] * 1e-3)
                yard = S * o["median_ms"]["ms_pairs"]
                c["yardstick_ms_pairs"] = yard
                c["ms_pairs_over_yardstick"] = c["median_ms"]["ms_pairs"] / yard
                c["beyond_spread_of_yardstick"] = abs(c["ms_pairs_over_yardstick"] - 1.0) > max(c["spread_pairs"], o["spread_pairs"])
                doc["topn"].append({"topn": t, "chain": c, "one_draw": o})
            out.append(doc)
            print(json.dumps(doc), flush=True)
            for h in (cs, cs1, m, one):
                h.close()
    return out


def serving(vbfm, synth, a):
    k, M, S = a.serve_k, a.serve_m, a.serve_draws
    D = max(M, (F - 1) * IDS) + 1
    m, one, _ = chain_and_draw(vbfm, k, D, S)
    one.close()
    cand = (np.arange(M + 1, dtype=np.uint64), np.arange(M, dtype=np.uint32), np.ones(M, dtype=np.float32))
    cs = m.candidates_chain(cand)
    rp, f, v, _ = synth.generate(1, F - 1, IDS, 302, 1)
    ms = []
    for r in range(a.rounds + 1):
        m.recommend_chain((rp, f, v), cs, 10, a.beta, noise=True, clip=False)
        if r:
            ms.append(m.last_recommend_stats["ms_pairs"])
    q_bytes = float(S) * M * k * 8
    doc = {"contexts": 1, "candidates": M, "k": k, "draws": S, "topn": 10, "q_bytes": q_bytes, "ms_pairs": ms,
           "median_ms": median(ms), "spread": spread(ms), "q_bytes_per_s": q_bytes / (median(ms) * 1e-3),
           "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE}
    doc["share_of_achievable"] = doc["q_bytes_per_s"] / HBM_ACHIEVABLE
    print(json.dumps(doc), flush=True)
    cs.close()
    m.close()
    return doc


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--contexts", type=int, default=65536)
    ap.add_argument("--baseline-contexts", type=int, default=40)
    ap.add_argument("--check-contexts", type=int, default=8)
    ap.add_argument("--k", type=int, nargs="+", default=[8, 20, 100])
    ap.add_argument("--draws", type=int, nargs="+", default=[8, 50])
    ap.add_argument("--topn", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--beta", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--serve-m", type=int, default=1_000_000)
    ap.add_argument("--serve-k", type=int, default=20)
    ap.add_argument("--serve-draws", type=int, default=8)
    ap.add_argument("--no-serving", action="store_true")
    ap.add_argument("--no-throughput", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_rank", "chain_rank_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("recommend_chain_bench.py needs a GPU")
    torch.cuda.init()
    import synth
    import vbfm
    doc = {"shape": {"fields": F, "ids_per_field": IDS}, "device": torch.cuda.get_device_name(0),
           "slices_override": os.environ.get("VBFM_REC_SLICES"), "context_tile": 8, "beta": a.beta, "noise": 1,
           "throughput": None if a.no_throughput else throughput(vbfm, synth, a),
           "serving": None if a.no_serving else serving(vbfm, synth, a)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()

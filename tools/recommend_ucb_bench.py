#!/usr/bin/env python3
"""Top-N by mean + beta * sd on one MI355X: vbfm_recommend_ucb against (1) the parent's only way to
the same answer -- every (context, candidate) pair expanded into one row and pushed through
vbfm_score with var -- and (2) vbfm_recommend, the mean-only ranking of the same inputs, which is its
floor (shapes and conventions of tools/recommend_bench.py, §12). All times are
device-event times the library reports.

Throughput regime. C3's feature space, 40 fields x 25,000 ids; --contexts (1e6) rows of the first 39
fields, the 25,000 ids of the last field as single-entry candidates. Per k in --k and topn in --topn:
    ucb        vbfm_recommend_ucb (beta --beta, noise 1) with each context tile in --tiles (8 16:
               VBFM_UCB_CTX), on a candidate set with the variance sums;
    mean       vbfm_recommend on that same set;
    baseline   --baseline-contexts (400) contexts expanded to 1e7 rows of 40 entries through
               vbfm_score(var), order = group, kernel time only.
    All alternate in one process, --rounds (3) rounds after a warm-up round; medians and spreads
    ((max - min) / median). check: the first --check-contexts (8) contexts' top-N recomputed from the
    baseline's means and variances.
Serving regime. B in --serve-b (1 64) against --serve-m (1e6) single-entry candidates, k = --serve-k
(100), topn 10: ms_pairs of both rankings.

Writes one JSON document to --out and prints it. Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from recommend_bench import F, S, expand, median, random_model   # noqa: E402  (it puts the package and tests on sys.path)

PHASES = ("ms_prepare", "ms_pairs", "ms_merge")


def spread(xs):
    return (max(xs) - min(xs)) / median(xs)


def timed(store, stats):
    for key in PHASES:
        store[key].append(stats[key])


def summary(store):
    med = {key: median(vals) for key, vals in store.items()}
    return {**store, "median_ms": med, "total_ms": sum(med.values()), "spread_pairs": spread(store["ms_pairs"])}


def set_tile(t):
    os.environ["VBFM_UCB_CTX"] = str(t)                  # read by the library at every call


def throughput(vbfm, synth, a):
    D = F * S + 1
    B = a.contexts
    rp, f, v, _ = synth.generate(B, F - 1, S, 301, 1)
    ctx = (rp, f, v)
    cand_ids = np.arange((F - 1) * S, F * S, dtype=np.uint32)
    M = len(cand_ids)
    cand = (np.arange(M + 1, dtype=np.uint64), cand_ids, np.ones(M, dtype=np.float32))
    nb = a.baseline_contexts
    base_rows = expand(ctx, cand_ids, nb)
    out = []
    for k in a.k:
        m = random_model(vbfm, k, D)
        cs = m.candidates(cand, variance=True)
        na = 1.0 / m.alpha
        new = lambda: {key: [] for key in PHASES}
        base_ms = []
        rec = {t: {"mean": new(), **{"ucb%d" % tile: new() for tile in a.tiles}} for t in a.topn}
        check = None
        for r in range(a.rounds + 1):                    # round 0 warms every kernel and buffer up
            mean, T = m.score(base_rows, variance=True, order="group", clip=False)
            if r:
                base_ms.append(m.last_stats["ms_kernel"])
            for t in a.topn:
                m.recommend(ctx, cs, t, clip=False)
                if r:
                    timed(rec[t]["mean"], m.last_recommend_stats)
                for tile in a.tiles:
                    set_tile(tile)
                    res = m.recommend_ucb(ctx, cs, t, a.beta, noise=True, clip=False)
                    if r:
                        timed(rec[t]["ucb%d" % tile], m.last_recommend_stats)
                    if r == 0 and t == a.topn[0] and tile == a.tiles[0]:   # the same answer as the baseline's
                        n = a.check_contexts
                        ref_m, ref_T = mean.reshape(nb, M)[:n], T.reshape(nb, M)[:n]
                        ref_k = ref_m + a.beta * np.sqrt(np.maximum(ref_T + na, 0.0))
                        top = np.sort(ref_k, axis=1)[:, ::-1][:, :t]
                        idx = res[0][:n].astype(np.int64)
                        rel = lambda x, y: float(np.max(np.abs(x - y) / np.maximum(1.0, np.abs(y))))
                        check = {"contexts": n, "topn": t, "beta": a.beta, "noise": 1,
                                 "rel_key_diff": rel(res[1][:n], top),
                                 "rel_diff_of_picked": rel(np.take_along_axis(ref_k, idx, axis=1), top),
                                 "rel_score_diff": rel(res[2][:n], np.take_along_axis(ref_m, idx, axis=1)),
                                 "rel_var_diff": rel(res[3][:n], np.take_along_axis(ref_T, idx, axis=1))}
                        check["within_1e-9"] = all(check[key] <= 1e-9 for key in check if key.startswith("rel_"))
        b = median(base_ms)
        base_pairs = nb * M / (b * 1e-3)
        doc = {"k": k, "contexts": B, "candidates": M, "pairs": B * M,
               "baseline": {"rows": nb * M, "ms_kernel": base_ms, "median_ms": b, "spread": spread(base_ms),
                            "pairs_per_s": base_pairs},
               "check": check, "topn": []}
        for t in a.topn:
            row = {"topn": t, "mean": summary(rec[t]["mean"])}
            for tile in a.tiles:
                s = summary(rec[t]["ucb%d" % tile])
                s["pairs_per_s"] = B * M / (s["total_ms"] * 1e-3)
                s["speedup_vs_baseline"] = s["pairs_per_s"] / base_pairs
                s["faster_by_more_than_spread"] = s["pairs_per_s"] > base_pairs * (1 + doc["baseline"]["spread"])
                s["ms_pairs_over_mean"] = s["median_ms"]["ms_pairs"] / row["mean"]["median_ms"]["ms_pairs"]
                s["pair_kernel_fma_per_s"] = 3.0 * B * M * k / (s["median_ms"]["ms_pairs"] * 1e-3)
                row["ucb%d" % tile] = s
            doc["topn"].append(row)
        out.append(doc)
        print(json.dumps(doc), flush=True)
        cs.close()
        m.close()
    return out


def serving(vbfm, synth, a):
    k, M = a.serve_k, a.serve_m
    D = max(M, (F - 1) * S) + 1
    m = random_model(vbfm, k, D)
    cand = (np.arange(M + 1, dtype=np.uint64), np.arange(M, dtype=np.uint32), np.ones(M, dtype=np.float32))
    cs = m.candidates(cand, variance=True)
    out = []
    for B in a.serve_b:
        rp, f, v, _ = synth.generate(B, F - 1, S, 302, 1)
        ms = {"mean": [], **{"ucb%d" % tile: [] for tile in a.tiles}}
        for r in range(a.rounds + 1):
            m.recommend((rp, f, v), cs, 10, clip=False)
            if r:
                ms["mean"].append(m.last_recommend_stats["ms_pairs"])
            for tile in a.tiles:
                set_tile(tile)
                m.recommend_ucb((rp, f, v), cs, 10, a.beta, noise=True, clip=False)
                if r:
                    ms["ucb%d" % tile].append(m.last_recommend_stats["ms_pairs"])
        doc = {"contexts": B, "candidates": M, "k": k, "topn": 10, "ms_pairs": ms,
               "median_ms": {key: median(v_) for key, v_ in ms.items()}}
        for tile in a.tiles:
            doc["ucb%d_over_mean" % tile] = doc["median_ms"]["ucb%d" % tile] / doc["median_ms"]["mean"]
            doc["ucb%d_cand_bytes_per_s" % tile] = 3.0 * M * k * 8 / (doc["median_ms"]["ucb%d" % tile] * 1e-3)
        out.append(doc)
        print(json.dumps(doc), flush=True)
    cs.close()
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--contexts", type=int, default=1_000_000)
    ap.add_argument("--baseline-contexts", type=int, default=400)
    ap.add_argument("--check-contexts", type=int, default=8)
    ap.add_argument("--k", type=int, nargs="+", default=[8, 16, 32, 100])
    ap.add_argument("--topn", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--tiles", type=int, nargs="+", default=[8, 16], choices=[8, 16])
    ap.add_argument("--beta", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--serve-b", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--serve-m", type=int, default=1_000_000)
    ap.add_argument("--serve-k", type=int, default=100)
    ap.add_argument("--no-serving", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recommend", "recommend_ucb_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("recommend_ucb_bench.py needs a GPU")
    torch.cuda.init()
    import synth
    import vbfm
    doc = {"shape": {"fields": F, "ids_per_field": S}, "device": torch.cuda.get_device_name(0),
           "slices_override": os.environ.get("VBFM_REC_SLICES"), "tiles": a.tiles, "beta": a.beta, "noise": 1,
           "throughput": throughput(vbfm, synth, a), "serving": None if a.no_serving else serving(vbfm, synth, a)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()

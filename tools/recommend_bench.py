#!/usr/bin/env python3
"""Top-N recommendation throughput on one MI355X: vbfm_recommend against the parent's way of doing
the same job -- every (context, candidate) pair expanded into one row and pushed through vbfm_score
(DESIGN.md §12). All times are device-event times the library reports.

Throughput regime. C3's feature space, 40 fields x 25,000 ids. Contexts: --contexts (1e6) rows of the
first 39 fields (tests/synth.py), x != 1, in host memory. Candidates: the 25,000 ids of the last
field, one entry each. Per k in --k (8 16 32 100) and topn in --topn (10 100):
    candidate  vbfm_recommend; ms_prepare / ms_pairs / ms_merge summed over the call's chunks;
               pairs/s = B * M over their sum, FMA/s = B * M * k over ms_pairs;
    baseline   --baseline-contexts (400) of the contexts expanded to 400 * 25,000 = 1e7 rows of 40
               entries (4e8 entries, tools/score_bench.py's size) through vbfm_score, order = group;
               kernel time only (ms_kernel): neither the copies nor the host-side sort a ranking
               would still need are charged, which favours the baseline. pairs/s = rows / ms_kernel.
    Baseline and candidates alternate in one process, --rounds (3) rounds after a warm-up round.
    Reported: every time, the medians, the baseline's spread (max - min over median) and whether
    the candidate's pairs/s beats the baseline's by more than that spread.
    Same results: the first --check-contexts (8) sub-sampled contexts' top-N recomputed from the
    baseline's scores of their expanded rows (1e-9 relative, the reordered-sum bound).

Serving regime. B in --serve-b (1 64) contexts against --serve-m (1e6) single-entry candidates (ids
0 .. M - 1), k = --serve-k (100), topn 10: ms_pairs and the bytes/s of streaming Q_cand (M * k * 8)
against the guides' achievable HBM rate (6.0-6.3 TB/s measured of 8 TB/s).

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

F, S = 40, 25000
HBM_ACHIEVABLE = 6.29e12   # bytes/s, float4 copy (the microarchitecture guide)


def median(xs):
    return float(np.median(np.asarray(xs, dtype=np.float64)))


def random_model(vbfm, k, D):
    fml = vbfm.FMLearnVB(1, 1, k, D, min_target=1.0, max_target=5.0, layout="column")
    fml.init_device(11)
    m = vbfm.Model.from_learner(fml)
    fml.close()
    return m


def expand(ctx, cand_ids, n_ctx):
    """Rows (context c's 39 entries, then candidate j's one), context-major: [n_ctx * M] rows of F."""
    rp, f, v = ctx
    M = len(cand_ids)
    feat = np.empty((n_ctx, M, F), dtype=np.uint32)
    val = np.empty((n_ctx, M, F), dtype=np.float32)
    feat[:, :, :F - 1] = f[:n_ctx * (F - 1)].reshape(n_ctx, 1, F - 1)
    val[:, :, :F - 1] = v[:n_ctx * (F - 1)].reshape(n_ctx, 1, F - 1)
    feat[:, :, F - 1] = cand_ids[None, :]
    val[:, :, F - 1] = 1.0
    return np.arange(n_ctx * M + 1, dtype=np.uint64) * np.uint64(F), feat.ravel(), val.ravel()


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
        cs = m.candidates(cand)
        base_ms, rec = [], {t: {"ms_prepare": [], "ms_pairs": [], "ms_merge": []} for t in a.topn}
        scores = None
        for r in range(a.rounds + 1):                  # round 0 warms every kernel and buffer up
            scores = m.score(base_rows, order="group", clip=False)
            if r:
                base_ms.append(m.last_stats["ms_kernel"])
            for t in a.topn:
                res = m.recommend(ctx, cs, t, clip=False)
                if r:
                    for key in rec[t]:
                        rec[t][key].append(m.last_recommend_stats[key])
                if r == 0 and t == a.topn[0]:          # same results as the baseline's scores
                    ref = scores.reshape(nb, M)[:a.check_contexts]
                    top = np.sort(ref, axis=1)[:, ::-1][:, :t]
                    rel = float(np.max(np.abs(res[1][:a.check_contexts] - top) / np.maximum(1.0, np.abs(top))))
                    picked = np.take_along_axis(ref, res[0][:a.check_contexts].astype(np.int64), axis=1)
                    rel_idx = float(np.max(np.abs(picked - top) / np.maximum(1.0, np.abs(top))))
        b = median(base_ms)
        spread = (max(base_ms) - min(base_ms)) / b
        base_pairs = nb * M / (b * 1e-3)
        doc = {"k": k, "contexts": B, "candidates": M, "pairs": B * M,
               "baseline": {"rows": nb * M, "ms_kernel": base_ms, "median_ms": b, "spread": spread, "pairs_per_s": base_pairs},
               "check": {"contexts": a.check_contexts, "rel_score_diff": rel, "rel_diff_of_picked": rel_idx,
                         "within_1e-9": rel <= 1e-9 and rel_idx <= 1e-9}, "topn": []}
        for t in a.topn:
            med = {key: median(vals) for key, vals in rec[t].items()}
            total = sum(med.values())
            pps = B * M / (total * 1e-3)
            doc["topn"].append({"topn": t, **rec[t], "median_ms": med, "pairs_per_s": pps,
                                "pair_kernel_fma_per_s": B * M * k / (med["ms_pairs"] * 1e-3),
                                "speedup_vs_baseline": pps / base_pairs,
                                "faster_by_more_than_spread": pps > base_pairs * (1 + spread)})
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
    cs = m.candidates(cand)
    out = []
    for B in a.serve_b:
        rp, f, v, _ = synth.generate(B, F - 1, S, 302, 1)
        ms = []
        for r in range(a.rounds + 1):
            m.recommend((rp, f, v), cs, 10, clip=False)
            if r:
                ms.append(m.last_recommend_stats["ms_pairs"])
        b = median(ms)
        rate = M * k * 8 / (b * 1e-3)
        out.append({"contexts": B, "candidates": M, "k": k, "topn": 10, "ms_pairs": ms, "median_ms": b,
                    "q_cand_bytes_per_s": rate, "share_of_achievable_hbm": rate / HBM_ACHIEVABLE})
        print(json.dumps(out[-1]), flush=True)
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--serve-b", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--serve-m", type=int, default=1_000_000)
    ap.add_argument("--serve-k", type=int, default=100)
    ap.add_argument("--no-serving", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recommend", "recommend_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("recommend_bench.py needs a GPU")
    torch.cuda.init()
    import synth
    import vbfm
    doc = {"shape": {"fields": F, "ids_per_field": S}, "device": torch.cuda.get_device_name(0),
           "slices_override": os.environ.get("VBFM_REC_SLICES"),
           "throughput": throughput(vbfm, synth, a), "serving": None if a.no_serving else serving(vbfm, synth, a)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()

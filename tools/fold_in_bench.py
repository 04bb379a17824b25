#!/usr/bin/env python3
"""vbfm_fold_in on one MI355X: --columns (1e5) new attributes x {5, 20, 200} rows,
k in {8, 20, 50, 100}, 20 passes, every lane width the auto rule could pick around each shape, so the
width table of csrc/vbfm_fold_plan.h is chosen from data.

Per (rows per column, k, width): ms_prepare and ms_fold (device time by events, summed over the
chunks), the median of --rounds calls after a warm-up call; columns/s of ms_fold; the A/B bytes the
sweep streams per pass (rows * k * 16) and that rate over ms_fold against 8 TB/s. Support rows hold
3 frozen ids and the new one, x != 1. The model is synthetic (D = 75,000).

Comparator on existing code, per (rows per column, k): one vbfm_iterate of a VB context that holds
the same rows as its train set (all ids, the new ones included): what a user pays per iteration to
learn the new ids by retraining.

Writes one JSON document to --out and prints it. Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scalable-variational-bayesian-factorization-machine_amd"))

D, FROZEN = 75000, 3
WIDTHS = {5: (4, 8, 16), 20: (8, 16, 32, 64), 200: (32, 64, 256)}


def support(columns, per, seed):
    rng = np.random.default_rng(seed)
    n = columns * per
    feat = np.empty((n, FROZEN + 1), dtype=np.uint32)
    for f in range(FROZEN):
        feat[:, f] = rng.integers(f * (D // FROZEN), (f + 1) * (D // FROZEN), size=n)
    feat[:, FROZEN] = D + rng.permutation(np.repeat(np.arange(columns), per))
    val = (0.5 + rng.random((n, FROZEN + 1))).astype(np.float32)
    y = rng.integers(1, 6, size=n).astype(np.float32)
    rp = np.arange(n + 1, dtype=np.uint64) * np.uint64(FROZEN + 1)
    return rp, feat.ravel(), val.ravel(), y


def model_file(vbfm, path, k, seed):
    rng = np.random.default_rng(seed)
    info = dict(kind=0, k0=1, k1=1, num_factor=k, num_attribute=D, min_target=1.0, max_target=5.0, iter=1, has_variance=1,
                w0_or_mu0=3.0, sigma_0_dash=0.01, alpha=1.5)
    p = dict(mu_w=0.3 * rng.standard_normal(D), sigma_w=0.01 + 0.05 * rng.random(D),
             mu_v=0.3 / np.sqrt(k) * rng.standard_normal(k * D), sigma_v=(0.01 + 0.05 * rng.random(k * D)) / k)
    vbfm.Model.write_params(path, info, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--columns", type=int, default=100000)
    ap.add_argument("--rows", type=int, nargs="*", default=[5, 20, 200])
    ap.add_argument("--k", type=int, nargs="*", default=[8, 20, 50, 100])
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fold_in", "fold_in_bench.json"))
    a = ap.parse_args()
    import vbfm
    doc = {"columns": a.columns, "passes": a.passes, "rounds": a.rounds, "D": D, "frozen_per_row": FROZEN, "fold": [], "retrain": []}
    tmp = os.path.join(os.path.dirname(a.out), ".model.tmp")
    for per in a.rows:
        rp, feat, val, y = support(a.columns, per, 100 + per)
        n = len(y)
        ds = vbfm.DataSubset.from_csr(rp, feat, val, y, D + a.columns)
        for k in a.k:
            model_file(vbfm, tmp, k, k)
            m = vbfm.Model.load(tmp)
            auto = None
            for g in (0,) + WIDTHS[per]:
                runs = []
                for r in range(a.rounds + 1):          # the first call warms up (staging buffers, code objects)
                    ext, st = m.fold_in((rp, feat, val, y), passes=a.passes, lanes=g)
                    ext.close()
                    runs.append(st)
                if g == 0:
                    auto = runs[-1]["lanes"]
                    continue
                prep = float(np.median([s["ms_prepare"] for s in runs[1:]]))
                fold = float(np.median([s["ms_fold"] for s in runs[1:]]))
                total = float(np.median([s["ms_total"] for s in runs[1:]]))
                ab = n * k * 16
                doc["fold"].append({"rows_per_column": per, "k": k, "lanes": g, "auto": g == auto, "ms_prepare": prep, "ms_fold": fold,
                                    "ms_total_host": total, "n_chunks": runs[-1]["n_chunks"], "columns_per_s": a.columns / (fold * 1e-3),
                                    "ab_bytes_per_pass": ab, "ab_bytes_per_s": ab * a.passes / (fold * 1e-3),
                                    "of_8TBps": ab * a.passes / (fold * 1e-3) / 8e12})
                print(json.dumps(doc["fold"][-1]), flush=True)
            m.close()
            # what a user pays today: one iteration of a VB context over the same rows
            fml = vbfm.FMLearnVB(1, 1, k, D + a.columns, min_target=1.0, max_target=5.0)
            fml.init(5, 0.1)
            fml.set_data(ds, ds)
            fml.init_caches()
            fml.iterate()
            ms = []
            for _ in range(a.rounds):
                st = fml.iterate()
                ms.append(st.ms_total)
            doc["retrain"].append({"rows_per_column": per, "k": k, "ms_iterate": float(np.median(ms))})
            print(json.dumps(doc["retrain"][-1]), flush=True)
            del fml
            with open(a.out, "w") as fh:       # after every shape: a run cut short keeps what it measured
                json.dump(doc, fh, indent=1)
                fh.write("\n")
    os.remove(tmp)


if __name__ == "__main__":
    main()

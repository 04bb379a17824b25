#!/usr/bin/env python3
"""What binary classification (-task c) adds to an MCMC / ALS iteration on one MI355X: the row
step after the re-prediction (k_mc_class_train_update / k_mc_class_test_update) against
regression's k_mc_train_update / k_mc_test_update on the same data, the same build and in the same
process. Both pairs move the same bytes per row: 8 B yhat, 4 B target, 4 B
position, one scattered record write.

Shape: --rows (1e7) x 40 one-hot fields x 25,000 ids, k = --k (16), generated on the device; the
classification targets are the same set binarized at the planted model's median (taken from a
200,000-row sample of the same model).

  c_mcmc   task c, -method mcmc, VBFM_RNG_DEVICE (the truncated normals drawn in the kernel)
  c_als    task c, -method als (the truncated expectation)
  r_mcmc   task r, -method mcmc, VBFM_RNG_DEVICE: the yardstick

Each run: one warm-up iteration, then --iters (3) timed ones; reported per iteration:
vbfm_mcmc_stats::ms_predict (device events around the re-prediction of test and train, the row
step and its reductions) and ms_total. The kernels' own device time comes from a separate run of
this tool under `rocprofv3 --kernel-trace --stats` (tracing slows the host, so not from this one).
--only r runs the yardstick alone and uses nothing a build without task c lacks, so the same file
times the parent commit's library.

Writes one JSON document to --out and prints it. Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scalable-variational-bayesian-factorization-machine_amd"))

F, S = 40, 25000
SAMPLE_ROWS = 200_000


def median_target(vbfm):
    """The planted model's median target, from a sample of rows of the same model."""
    fml = vbfm.FMLearnMCMC(1, 1, 1, F * S + 1, method="als")
    fml.synth(0, SAMPLE_ROWS, F, S, 77, xmode=1)
    y = fml.get_csc(0)[2]
    fml.close()
    return float(np.median(y))


def one_run(vbfm, name, rows, test_rows, k, iters, threshold):
    task, method = ("c" if name.startswith("c_") else "r"), name.split("_")[1]
    kw = {"task": "c"} if task == "c" else {}
    lo, hi = (-1.0, 1.0) if task == "c" else (1.0, 5.0)
    fml = vbfm.FMLearnMCMC(1, 1, k, F * S + 1, min_target=lo, max_target=hi, method=method, **kw)
    fml.init_device(11, 0.1)
    fml.synth(0, rows, F, S, 101, xmode=1)
    fml.synth(1, test_rows, F, S, 102, xmode=1)
    out = {"task": task, "method": method, "layout": None}
    if task == "c":
        out["positives"] = fml.synth_binarize(0, threshold) / rows
        fml.synth_binarize(1, threshold)
    fml.init_caches()
    fml.iterate()   # warm-up: code objects, the store, the placement search
    out["layout"] = fml.layout()
    ms_predict, ms_total, acc = [], [], []
    for _ in range(iters):
        st = fml.iterate()
        ms_predict.append(st.ms_predict)
        ms_total.append(st.ms_total)
        if task == "c":
            ci = fml.class_info()
            acc.append(ci["acc_train"])
            assert ci["nonfinite_rows"] == 0 and ci["capped_rows"] == 0, ci
    out.update(ms_predict=ms_predict, ms_total=ms_total, ms_predict_median=float(np.median(ms_predict)),
               ms_predict_spread=(max(ms_predict) - min(ms_predict)) / float(np.median(ms_predict)))
    if acc:
        out["acc_train"] = acc
    fml.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--test-rows", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--only", default="", help="r: the regression yardstick alone")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "class_bench needs a GPU"
    torch.cuda.init()
    import vbfm
    names = ["r_mcmc"] if a.only == "r" else ["c_mcmc", "c_als", "r_mcmc"]
    threshold = median_target(vbfm) if a.only != "r" else None
    doc = {"rows": a.rows, "test_rows": a.test_rows, "fields": F, "ids_per_field": S, "k": a.k, "iters": a.iters,
           "threshold": threshold, "runs": {}}
    for name in names:
        doc["runs"][name] = one_run(vbfm, name, a.rows, a.test_rows, a.k, a.iters, threshold)
    r = doc["runs"]["r_mcmc"]["ms_predict_median"]
    for name in names:
        if name != "r_mcmc":
            doc["runs"][name]["ms_predict_over_r"] = doc["runs"][name]["ms_predict_median"] / r
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Scoring throughput on one MI355X: the lane-group scoring kernel (vbfm_score_device) against the
training path's wave-per-row test prediction (k_predict_e_wave) on the same rows and the same
build, and vbfm_score's chunked pass over host-resident rows.

Shape: C3's, generated on the device: --rows (1e7) x 40 fields x 25,000 ids per field, x != 1.

  device-resident, per k in --k (8, 32, 100):
    baseline   the rows attached as the TEST set of a context (a small train set beside them), one
               vbfm_iterate with VBFM_PREDICT=wave, vbfm_iter_stats::ms_test_predict;
    candidate  vbfm_score_device's ms_kernel on the same rows, order = group, mean only and with T
               (and, as an A/B of the group size alone, the same two with VBFM_SCORE_G=64: one row
               per wave).
    Baseline and candidates alternate in one process, --rounds (3) rounds after a warm-up. Reported:
    the three times of each, rows/s and bytes/s of the median, the baseline's spread (max - min
    over median) and whether each candidate is within that spread of the baseline or faster.
    bytes = nnz * k * 8 (mean table; 16 with T, and for the baseline, which gathers the
    {mu, sigma} pairs) + the CSR's bytes (8 per entry + 8 per row), over kernel time.
  host-resident (--host-k, 8): the same rows read back to host memory and scored through
    vbfm_score at each --chunks value: ms_copy, ms_kernel, ms_total, rows/s of ms_total.

Writes one JSON document to --out and prints it. Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scalable-variational-bayesian-factorization-machine_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

F, S = 40, 25000


def median(xs):
    return float(np.median(np.asarray(xs, dtype=np.float64)))


def rates(ms, rows, nnz, k, per_factor):
    s = ms * 1e-3
    gathered = nnz * k * per_factor
    return {"ms": ms, "rows_per_s": rows / s, "gathered_bytes_per_s": gathered / s,
            "bytes_per_s": (gathered + nnz * 8 + rows * 8) / s}


def device_pass(vbfm, k, rows, train_rows, rounds):
    D = F * S + 1
    fml = vbfm.FMLearnVB(1, 1, k, D, min_target=1.0, max_target=5.0, layout="column")
    fml.init_device(11)
    fml.synth(0, train_rows, F, S, 101, xmode=1)
    fml.synth(1, rows, F, S, 102, xmode=1)
    nnz = fml.shape(1)[2]
    fml.init_caches()
    model = vbfm.Model.from_learner(fml)
    base, mean_only, with_var, mean_g64, var_g64 = [], [], [], [], []

    def timed(variance):
        model.score_device(fml, 1, variance=variance, order="group")
        return model.last_stats["ms_kernel"]

    for r in range(rounds + 1):                      # round 0 warms every kernel up
        st = fml.iterate()
        t_mean, t_var = timed(False), timed(True)
        os.environ["VBFM_SCORE_G"] = "64"            # the same kernels at one row per wave (A/B)
        t_mean64, t_var64 = timed(False), timed(True)
        del os.environ["VBFM_SCORE_G"]
        if r:
            base.append(st.ms_test_predict)
            mean_only.append(t_mean)
            with_var.append(t_var)
            mean_g64.append(t_mean64)
            var_g64.append(t_var64)
    # same results: the candidate on the parameters the last baseline prediction read
    last = vbfm.Model.from_learner(fml)
    got, ref = last.score_device(fml, 1, order="group", clip=False), fml.test_e()
    same = bool(np.array_equal(got.view(np.uint64), ref.view(np.uint64)))
    rel = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
    b = median(base)
    spread = (max(base) - min(base)) / b
    out = {"k": k, "rows": rows, "nnz": nnz, "baseline_ms": base, "mean_ms": mean_only, "var_ms": with_var,
           "baseline": rates(b, rows, nnz, k, 16), "baseline_spread": spread,
           "mean": rates(median(mean_only), rows, nnz, k, 8), "var": rates(median(with_var), rows, nnz, k, 16),
           "mean_one_row_per_wave_ms": mean_g64, "var_one_row_per_wave_ms": var_g64,
           "mean_vs_baseline": median(mean_only) / b, "var_vs_baseline": median(with_var) / b,
           "mean_within_spread_or_faster": median(mean_only) <= b * (1 + spread),
           "var_within_spread_or_faster": median(with_var) <= b * (1 + spread),
           "bit_identical_to_baseline": same, "rel_diff_to_baseline": rel}
    last.close()
    model.close()
    return out, fml


def host_pass(vbfm, synth, fml, k, rows, chunks):
    t0 = time.time()
    cp, ent, _ = fml.get_csc(1)
    rp, feat, val = synth.field_csr_from_csc(rows, F, S, cp, ent["id"], ent["value"])
    del cp, ent
    readback_s = time.time() - t0
    model = vbfm.Model.from_learner(fml)
    ref = model.score_device(fml, 1, order="group")
    out = {"k": k, "rows": rows, "readback_s": readback_s, "chunks": []}
    for cb in chunks:
        best = None
        for _ in range(2):                           # the first call allocates the staging buffers
            got = model.score((rp, feat, val), order="group", chunk_bytes=cb)
            st = dict(model.last_stats)
            if best is None or st["ms_total"] < best["ms_total"]:
                best = st
        best.update(chunk_bytes=cb, rows_per_s=rows / (best["ms_total"] * 1e-3),
                    bit_identical_to_device_resident=bool(np.array_equal(got.view(np.uint64), ref.view(np.uint64))))
        out["chunks"].append(best)
    model.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--train-rows", type=int, default=100_000)
    ap.add_argument("--k", type=int, nargs="+", default=[8, 32, 100])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-k", type=int, default=8)
    ap.add_argument("--chunks", type=int, nargs="+", default=[16 << 20, 64 << 20, 256 << 20])
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score", "score_bench.json"))
    a = ap.parse_args()
    os.environ["VBFM_PREDICT"] = "wave"
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("score_bench.py needs a GPU")
    torch.cuda.init()
    import synth
    import vbfm
    doc = {"shape": {"rows": a.rows, "fields": F, "ids_per_field": S}, "device": torch.cuda.get_device_name(0),
           "device_resident": [], "host_resident": None}
    for k in a.k:
        res, fml = device_pass(vbfm, k, a.rows, a.train_rows, a.rounds)
        doc["device_resident"].append(res)
        print(json.dumps(res), flush=True)
        if k == a.host_k and not a.no_host:
            doc["host_resident"] = host_pass(vbfm, synth, fml, k, a.rows, a.chunks)
            print(json.dumps(doc["host_resident"]), flush=True)
        fml.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Scoring a chain of S draws on one MI355X: one call on a chain model (k_score_chain on the
interleaved tables) against the parent's way of doing the same job -- S one-draw
models scored by S vbfm_score_device calls on the same device-resident rows, their scores averaged
on the host. All times are the device-event kernel times the library reports (ms_kernel).

Shapes, generated on the device (tests/synth.py's generator), x != 1:
    c2   ML-1M's shape: 2 fields x 5,000 ids, --c2-rows (1e6) rows, k in --c2-k (8 20);
    c3   C3's feature space: 40 fields x 25,000 ids, --c3-rows (1e6) rows -- a row count that fits
         beside 32 draws of k = 100 twice over (the chain and the one-draw models) -- k in --c3-k (50 100).
Per (shape, k) and S in --draws (8 32): the draws are S contexts' device-initialised parameters
(VBFM_RNG_DEVICE, one seed each), added to a collector and snapshot as one-draw models.
    baseline   S vbfm_score_device calls (order = group, clipped), kernel times summed; the host-side
               averaging is not charged, which favours the baseline;
    candidate  one vbfm_score_device call on the chain model (order = group, clipped): the means
               alone, which is what the baseline produces, and -- reported beside it -- with var;
               both of its geometries (VBFM_CHAIN_LOOP=0: the draws across the wave, =1: the per-draw
               loop, a lane group taking its row's draws one after another as k_score takes rows),
               and once more as the library dispatches on its own ("chain_ms" is that one).
    Baseline and candidate alternate in one process, --rounds (3) rounds after a warm-up round.
    Reported: every time, the medians, each side's spread (max - min over median), the ratio, and
    whether the candidate is faster than the baseline beyond the larger of the two spreads.
    Same results: the candidate's mean and var against the float64 restatement of the definition
    (include/vbfm.h "chains of draws") over the baseline's per-draw scores, bit for bit.

Writes one JSON document to --out and prints it. Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scalable-variational-bayesian-factorization-machine_amd"))

SHAPES = {"c2": (2, 5000), "c3": (40, 25000)}
MN, MX = 1.0, 5.0


def median(xs):
    return float(np.median(np.asarray(xs, dtype=np.float64)))


def spread(xs):
    return (max(xs) - min(xs)) / median(xs)


def restate(p):
    """mean (clipped to the target range) and var of the definition, from the per-draw clipped scores."""
    S = len(p)
    total = np.zeros_like(p[0])
    for s in range(S):
        total = total + p[s]
    mean = np.maximum(MN, np.minimum(MX, total / S))
    m, M2 = np.zeros_like(p[0]), np.zeros_like(p[0])
    for s in range(S):
        d = p[s] - m
        m = m + d / (s + 1)
        M2 = M2 + d * (p[s] - m)
    return mean, M2 / S


def learner(vbfm, k, D, seed):
    fml = vbfm.FMLearnMCMC(1, 1, k, D, min_target=MN, max_target=MX, method="mcmc", layout="column")
    fml.init(seed, 0.1, rng=vbfm.RNG_DEVICE)
    return fml


def one_k(vbfm, name, k, rows, draws, rounds):
    F, ids = SHAPES[name]
    D = F * ids + 1
    data = learner(vbfm, k, D, 1)
    data.synth(1, rows, F, ids, 102, xmode=1)
    nnz = data.shape(1)[2]
    smax = max(draws)
    chains = {S: data.chain(S) for S in draws}
    ones = []
    for s in range(smax):
        fml = learner(vbfm, k, D, 100 + s)
        for S, ch in chains.items():
            if s < S:
                ch.add(fml)
        ones.append(vbfm.Model.from_learner(fml))
        fml.close()
    out = []
    for S in draws:
        model = chains[S].model()
        chains[S].close()
        base, cand, cand_var = [], [], []
        forced, forced_out = {"wave": ([], []), "loop": ([], [])}, {}
        per_draw = got = None
        for r in range(rounds + 1):                  # round 0 warms every kernel up
            t, per_draw = 0.0, []
            for m in ones[:S]:
                per_draw.append(m.score_device(data, 1, order="group"))
                t += m.last_stats["ms_kernel"]
            for name_v, env in (("wave", "0"), ("loop", "1")):   # the two geometries, forced (A/B)
                os.environ["VBFM_CHAIN_LOOP"] = env
                o_mean = model.score_device(data, 1, order="group")
                t_m = model.last_stats["ms_kernel"]
                o_var = model.score_device(data, 1, variance=True, order="group")
                if r:
                    forced[name_v][0].append(t_m)
                    forced[name_v][1].append(model.last_stats["ms_kernel"])
                forced_out[name_v] = (o_mean, o_var)
            del os.environ["VBFM_CHAIN_LOOP"]                    # ... and the library's own dispatch
            mean_only = model.score_device(data, 1, order="group")
            t_mean = model.last_stats["ms_kernel"]
            got = model.score_device(data, 1, variance=True, order="group")
            if r:
                base.append(t)
                cand.append(t_mean)
                cand_var.append(model.last_stats["ms_kernel"])
        em, ev = restate(per_draw)
        same = bool(np.array_equal(got[0].view(np.uint64), em.view(np.uint64)) and
                    np.array_equal(got[1].view(np.uint64), ev.view(np.uint64)) and
                    np.array_equal(mean_only.view(np.uint64), em.view(np.uint64)))
        for o_mean, o_var in forced_out.values():
            same = same and bool(np.array_equal(o_mean.view(np.uint64), em.view(np.uint64)) and
                                 np.array_equal(o_var[0].view(np.uint64), em.view(np.uint64)) and
                                 np.array_equal(o_var[1].view(np.uint64), ev.view(np.uint64)))
        b, c = median(base), median(cand)
        noise = max(spread(base), spread(cand))
        res = {"shape": name, "k": k, "draws": S, "rows": rows, "nnz": nnz, "baseline_ms": base, "chain_ms": cand,
               "chain_with_var_ms": cand_var, "chain_with_var_median_ms": median(cand_var),
               "chain_with_var_over_baseline": median(cand_var) / b,
               "wave_ms": forced["wave"][0], "wave_with_var_ms": forced["wave"][1],
               "loop_ms": forced["loop"][0], "loop_with_var_ms": forced["loop"][1],
               "wave_over_baseline": median(forced["wave"][0]) / b, "loop_over_baseline": median(forced["loop"][0]) / b,
               "wave_with_var_over_baseline": median(forced["wave"][1]) / b,
               "loop_with_var_over_baseline": median(forced["loop"][1]) / b,
               "baseline_median_ms": b, "chain_median_ms": c, "baseline_spread": spread(base), "chain_spread": spread(cand),
               "chain_over_baseline": c / b, "chain_faster_beyond_spread": bool(c < b * (1 - noise)),
               "gathered_bytes_per_s": nnz * (k + 1) * 8 * S / (c * 1e-3),
               "bit_identical_to_restated_baseline": same}
        print(json.dumps(res), flush=True)
        out.append(res)
        model.close()
    for m in ones:
        m.close()
    data.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--c2-rows", type=int, default=1_000_000)
    ap.add_argument("--c3-rows", type=int, default=1_000_000)
    ap.add_argument("--c2-k", type=int, nargs="*", default=[8, 20])
    ap.add_argument("--c3-k", type=int, nargs="*", default=[50, 100])
    ap.add_argument("--draws", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain", "chain_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("chain_bench.py needs a GPU")
    torch.cuda.init()
    import vbfm
    prop = torch.cuda.get_device_properties(0)
    doc = {"device": torch.cuda.get_device_name(0), "gcn_arch": getattr(prop, "gcnArchName", None),
           "compute_units": prop.multi_processor_count, "memory_bytes": prop.total_memory, "rounds": a.rounds, "results": []}
    for name, ks, rows in (("c2", a.c2_k, a.c2_rows), ("c3", a.c3_k, a.c3_rows)):
        for k in ks:
            doc["results"] += one_k(vbfm, name, k, rows, a.draws, a.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()

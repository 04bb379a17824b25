"""What tests/test_recommend_chain_gpu.py and tests/test_recommend_chain_cpu.py share: the case table of
the chain ranking (include/vbfm.h "ranking a chain of draws"), chain models written with
Model.write_chain from numpy draws, the tolerances of the comparison with the existing scorer, and a
plain numpy FM that values every (context, candidate) pair of a case for every draw. It builds on
tests/recommend_cases.py (contexts, candidates, expand, bits, same). The assertions are in the test
files."""
import numpy as np

import vbfm
from recommend_cases import D_SYNTH, MCMC_CHAIN, MCMC_DRAW

REL = 1e-9                        # the project's bound for a reordered fp64 sum (tests/test_score_gpu.py)
LOOSE_SHARE = 0.05                # of a case's pairs that may fall on the sqrt(tol_v) branch of tol_key
# the chain pair kernel's geometry (csrc/vbfm_recommend.hip): a wave owns CHAIN_CTX contexts, a workgroup
# CHAIN_TILE_B (the one tile compiled: DESIGN.md §16); a wave step takes REC_STEP candidates
CHAIN_CTX, CHAIN_TILE_B, REC_STEP = 8, 32, 128

# k through the G / pass boundaries of the preparation kernel; S through one draw, the smallest spread
# and counts on both sides of a power of two; B through the wave's and the workgroup's context tile
# +-1; M through the candidate step +-1, 2 steps + 1 and M < topn; topn through the three list
# capacities (16, 64, 128); beta, noise and the k0 / k1 combinations rotate; two cases are task c
CASES = [
    # k, k0, k1, S, B, M, topn, beta, noise, task
    (0, 1, 1, 1, CHAIN_CTX + 1, REC_STEP + 1, 10, 0.0, 0, "r"),
    (1, 0, 1, 2, 1, 1, 1, 2.0, 1, "r"),
    (7, 1, 0, 3, CHAIN_CTX - 1, REC_STEP - 1, 10, -1.0, 0, "r"),
    (8, 1, 1, 9, CHAIN_CTX, REC_STEP, 128, 0.5, 1, "r"),
    (9, 0, 0, 17, CHAIN_CTX + 1, REC_STEP + 1, 1, 0.0, 0, "c"),
    (16, 1, 1, 1, CHAIN_TILE_B + 1, REC_STEP + 1, 100, 2.0, 1, "r"),
    (33, 1, 1, 2, CHAIN_TILE_B - 1, 2 * REC_STEP + 1, 10, -1.0, 0, "r"),
    (64, 1, 1, 3, CHAIN_TILE_B, 5, 10, 0.5, 1, "r"),                      # M < topn: short lists, padding
    (65, 0, 1, 9, CHAIN_TILE_B + 1, 2 * REC_STEP - 1, 128, 2.0, 0, "c"),
    (100, 1, 1, 17, 3, 100, 128, 2.0, 1, "r"),                            # M < topn
    (100, 1, 0, 2, 1, 3 * REC_STEP, 64, -1.0, 0, "r"),
    (8, 1, 1, 2, CHAIN_CTX + 1, REC_STEP + 1, 64, 0.5, 0, "r"),           # S = 2, k = 8: the most small spreads
    (20, 1, 1, 1, CHAIN_CTX, REC_STEP - 1, 10, 2.0, 0, "r"),              # S = 1, noise = 0: key is score
]
CASE_IDS = ["k%d-S%d-B%d-M%d-n%d" % (c[0], c[3], c[4], c[5], c[6]) for c in CASES]


def chain_info(k, k0, k1, D=D_SYNTH, mn=-1.0, mx=1.5):
    return dict(kind=MCMC_CHAIN, k0=k0, k1=k1, num_factor=k, num_attribute=D, min_target=mn, max_target=mx, iter=1,
                has_variance=0, w0_or_mu0=0.0, sigma_0_dash=0.0, alpha=1.0)


def chain_draws(k, S, D=D_SYNTH, seed=1):
    """S independent draws: w, v ~ 0.3 N(0, 1), w0 = 0.37 + 0.1 s, alpha = 1 + s; v as [f][j]."""
    rng = np.random.default_rng(7000 * seed + 100 * S + k)
    return [dict(w=0.3 * rng.standard_normal(D), v=0.3 * rng.standard_normal(k * D), w0=0.37 + 0.1 * s, alpha=1.0 + s)
            for s in range(S)]


def write_chain(tmp_path, k, k0, k1, draws, task="r", D=D_SYNTH, mn=-1.0, mx=1.5, name="chain"):
    path = str(tmp_path / ("%s_%d_%d%d_%d_%s.vbfm" % (name, k, k0, k1, len(draws), task)))
    vbfm.Model.write_chain(path, chain_info(k, k0, k1, D, mn, mx), draws, task=task)
    return path


def make_chain(tmp_path, k, k0, k1, S, task="r", D=D_SYNTH, seed=1, mn=-1.0, mx=1.5, edit=None, name="chain"):
    """(model, file, draws) of a chain of S random draws; edit(draws) may change them before they are written."""
    draws = chain_draws(k, S, D, seed)
    if edit:
        edit(draws)
    path = write_chain(tmp_path, k, k0, k1, draws, task, D, mn, mx, name)
    return vbfm.Model.load(path), path, draws


def draw_model(tmp_path, chain_file, s, task="r", name="draw"):
    """The MCMC_DRAW model of draw s of a chain file, through Model.read_draw and Model.write_params."""
    p = vbfm.Model.read_draw(chain_file, s)
    info = dict(p["info"], kind=MCMC_DRAW, w0_or_mu0=p["w0"], alpha=p["alpha"])
    path = str(tmp_path / ("%s_%d.vbfm" % (name, s)))
    vbfm.Model.write_params(path, info, {"w": p["w"], "v": p["v"]}, task=task)
    return vbfm.Model.load(path)


def noise_term(draws, noise):
    """na: the mean over the draws of 1 / alpha_s, summed in draw order (0 without noise)."""
    if not noise:
        return 0.0
    s = 0.0
    for d in draws:
        s = s + 1.0 / d["alpha"]
    return s / len(draws)


def tolerances(mean, var, na, beta):
    """Per context tol_m and tol_v [B, 1], per pair tol_key [B, M] and the pairs on its loose branch, from the
    reference's mean and var [B, M]: tol_key = tol_m + |beta| min(sqrt(tol_v), tol_v / sqrt(var + na)), the
    exact bound on a difference of square roots whose arguments differ by tol_v."""
    fin = np.isfinite(mean) & np.isfinite(var)
    am = np.where(fin, np.abs(mean), 0.0)
    av = np.where(fin, var, 0.0)
    tol_m = REL * np.maximum(1.0, am.max(axis=1, keepdims=True) if mean.shape[1] else np.zeros((len(mean), 1)))
    tol_v = REL * np.maximum(1.0, av.max(axis=1, keepdims=True) if mean.shape[1] else np.zeros((len(mean), 1)))
    with np.errstate(divide="ignore", invalid="ignore"):
        tight = tol_v / np.sqrt(var + na)
    tight = np.where(np.isnan(tight), np.inf, tight)
    tol_key = tol_m + abs(beta) * np.minimum(np.sqrt(tol_v), tight)
    loose = fin & (var + na < 1e4 * tol_v)
    return tol_m, tol_v, tol_key, loose


def _sums(rows, D):
    """X [n, D] (the sum of a row's x per id) and X2 (the sum of x^2), float64."""
    rp, f, v = rows
    n = len(rp) - 1
    r = np.repeat(np.arange(n), np.diff(rp.astype(np.int64)))
    X, X2 = np.zeros((n, D)), np.zeros((n, D))
    x = v.astype(np.float64)
    np.add.at(X, (r, f.astype(np.int64)), x)
    np.add.at(X2, (r, f.astype(np.int64)), x * x)
    return X, X2


def numpy_raw(draws, k, k0, k1, ctx, cand, D=D_SYNTH):
    """raw [S, B, M]: the FM's value of the row holding context c's and candidate j's entries, for every
    draw, in plain numpy (no claim on the summation order)."""
    Xc, X2c = _sums(ctx, D)
    Xj, X2j = _sums(cand, D)
    out = np.zeros((len(draws), len(Xc), len(Xj)))
    for s, d in enumerate(draws):
        w, V = d["w"], d["v"].reshape(k, D).T                  # V [D, k]
        lin = (Xc @ w)[:, None] + (Xj @ w)[None, :] if k1 else 0.0
        Qc, Qj = Xc @ V, Xj @ V
        sq = (X2c @ (V * V)).sum(axis=1)[:, None] + (X2j @ (V * V)).sum(axis=1)[None, :]
        Q2 = (Qc * Qc).sum(axis=1)[:, None] + (Qj * Qj).sum(axis=1)[None, :] + 2.0 * (Qc @ Qj.T)
        out[s] = (d["w0"] if k0 else 0.0) + lin + 0.5 * (Q2 - sq)
    return out


def shifted_moments(raw):
    """include/vbfm.h's expressions of the chain's mean and var from raw [S, ...], restated in numpy
    operation by operation (numpy has no fma: b = b + d * d rounds twice, which the 1e-12 comparison of
    tests/test_recommend_chain_cpu.py does not see)."""
    S = raw.shape[0]
    invS = 1.0 / S
    a, b = np.zeros(raw.shape[1:]), np.zeros(raw.shape[1:])
    for s in range(1, S):
        d = raw[s] - raw[0]
        a = a + d
        b = b + d * d
    am = a * invS
    return raw[0] + am, np.maximum((b - a * am) * invS, 0.0)

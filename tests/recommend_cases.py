"""What tests/test_recommend_gpu.py and tests/test_recommend_ucb_gpu.py share: models written from numpy
arrays, context and candidate rows, the expansion of every (context, candidate) pair into one row for
the existing scorer, and bit-for-bit comparison. The references, tolerances and assertions are in the
test files."""
import numpy as np

import synth
import vbfm

F, S = 5, 50                      # contexts: synth.generate's 5 fields x 50 ids
D_SYNTH = F * S + 1               # id 250 is in the model and in no context
VB, VB_ONLINE, ALS, MCMC_DRAW, MCMC_CHAIN = 0, 1, 2, 3, 4
ALPHA = 1.5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """Two results of a ranking call -- (idx, score, count) or (idx, key, score, var, count) -- bit for bit."""
    return len(a) == len(b) and all(
        np.array_equal(bits(x), bits(y)) if x.dtype == np.float64 else np.array_equal(x, y) for x, y in zip(a, b))


def make_model(tmp_path, kind, k, k0, k1, D=D_SYNTH, seed=1, task="r", mn=-1.0, mx=1.5, edit=None, sig=0.05, name="m"):
    """A model of random parameters, loaded from the file <name>_<kind>_<k>_<k0><k1>_<task>.vbfm it is
    written to; VB kinds: sigma_w, sigma_v in [0.01, 0.01 + sig), sigma_0_dash 0.02. edit(p) may change
    the parameter arrays (p as Model.write_params takes them) before they are written."""
    rng = np.random.default_rng(1000 * seed + k)
    vbk = kind in (VB, VB_ONLINE)
    info = dict(kind=kind, k0=k0, k1=k1, num_factor=k, num_attribute=D, min_target=mn, max_target=mx, iter=1,
                has_variance=int(vbk), w0_or_mu0=0.37, sigma_0_dash=0.02 if vbk else 0.0, alpha=ALPHA)
    w, v = 0.3 * rng.standard_normal(D), 0.3 * rng.standard_normal(k * D)
    if vbk:
        p = {"mu_w": w, "sigma_w": 0.01 + sig * rng.random(D), "mu_v": v, "sigma_v": 0.01 + sig * rng.random(k * D)}
    else:
        p = {"w": w, "v": v}
    if edit:
        edit(p)
    path = str(tmp_path / ("%s_%d_%d_%d%d_%s.vbfm" % (name, kind, k, k0, k1, task)))
    vbfm.Model.write_params(path, info, p, task=task)
    return vbfm.Model.load(path)


_CTX = {}


def contexts(B, seed=3):
    """synth.generate rows (non-unit x), every third value negated."""
    if (B, seed) not in _CTX:
        rp, f, v, _ = synth.generate(B, F, S, seed, 1)
        v = v.copy()
        v[::3] *= -1.0
        _CTX[(B, seed)] = (rp, f, v)
    return _CTX[(B, seed)]


def candidates(M, seed=5, D=D_SYNTH):
    """M rows of 1-3 entries over the contexts' id range (so candidates share ids with contexts),
    non-unit and negative x, a repeated id now and then; row 1 (when there is one) is empty."""
    rng = np.random.default_rng(seed)
    n = rng.integers(1, 4, size=M)
    if M > 1:
        n[1] = 0
    rp = np.zeros(M + 1, dtype=np.uint64)
    np.cumsum(n, out=rp[1:])
    f = rng.integers(0, D - 1, size=int(rp[-1])).astype(np.uint32)
    v = (rng.standard_normal(int(rp[-1])) + 0.25).astype(np.float32)
    return rp, f, v


def expand(ctx, cand):
    """The B * M rows (context entries, then candidate entries), context-major."""
    crp, cf, cv = ctx
    jrp, jf, jv = cand
    B, M = len(crp) - 1, len(jrp) - 1
    crp, jrp = crp.astype(np.int64), jrp.astype(np.int64)
    fs, vs, lens = [], [], np.zeros(B * M, dtype=np.int64)
    for c in range(B):
        a_f, a_v = cf[crp[c]:crp[c + 1]], cv[crp[c]:crp[c + 1]]
        for j in range(M):
            fs += [a_f, jf[jrp[j]:jrp[j + 1]]]
            vs += [a_v, jv[jrp[j]:jrp[j + 1]]]
            lens[c * M + j] = len(a_f) + jrp[j + 1] - jrp[j]
    rp = np.zeros(B * M + 1, dtype=np.uint64)
    np.cumsum(lens, out=rp[1:])
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt)
    return rp, cat(fs, np.uint32), cat(vs, np.float32)

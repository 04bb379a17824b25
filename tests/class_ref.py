"""NumPy restatements of the reference's binary-classification arithmetic, written from its lines
(util/random.h:47-114, fm_learn_mcmc_simultaneous.h:176-221, 383-401), and the helpers the
classification tests share: the thresholded data sets and the fixture traces."""
import gzip
import json
import math
import os

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(TESTS, "golden")


def erf_ref(x):
    """random.h:47-61: the five-term polynomial that shadows libm's erf in the reference."""
    x = np.asarray(x, dtype=np.float64)
    t = np.where(x >= 0, 1.0 / (1.0 + 0.3275911 * x), 1.0 / (1.0 - 0.3275911 * x))
    r = 1.0 - (t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))) * \
        np.exp(-x * x)
    return np.where(x >= 0, r, -r)


def Phi(x):
    """cdf_gaussian (random.h:67-69)."""
    return 0.5 + 0.5 * erf_ref(0.707106781 * np.asarray(x, dtype=np.float64))


def phi_ref(mu):
    """:204 / :214, pi = 3.141 as written."""
    mu = np.asarray(mu, dtype=np.float64)
    return np.exp(-mu * mu / 2.0) / math.sqrt(3.141 * 2)


def expect_left(mu):
    """:203-206: the latent target of a row with target >= 0 under als."""
    return mu + phi_ref(mu) / (1 - Phi(-np.asarray(mu, dtype=np.float64)))


def expect_right(mu):
    """:213-216: ... with target < 0."""
    return mu - phi_ref(mu) / Phi(-np.asarray(mu, dtype=np.float64))


def expect_target(yhat, y):
    return np.where(np.asarray(y) >= 0, expect_left(yhat), expect_right(yhat))


def correct(p, y):
    """:193 / :389: a zero target is never correct."""
    p, y = np.asarray(p), np.asarray(y)
    return ((p >= 0.5) & (y > 0)) | ((p < 0.5) & (y < 0))


def loglik(p, y):
    """_evaluate_class (:383-401): mean of -(m log10 p + (1 - m) log10(1 - p)), p in [0.01, 0.99]."""
    m = (np.asarray(y, dtype=np.float64) + 1.0) * 0.5
    pll = np.clip(np.asarray(p, dtype=np.float64), 0.01, 0.99)
    return float(np.mean(-(m * np.log10(pll) + (1 - m) * np.log10(1 - pll))))


def trunc_moments(mu):
    """Mean, variance and fourth central moment of N(mu, 1) truncated to [0, inf), exact Phi (erfc)."""
    a = -mu
    tail = 0.5 * math.erfc(a / math.sqrt(2.0))
    lam = math.exp(-a * a / 2.0) / math.sqrt(2.0 * math.pi) / tail
    mean = mu + lam
    var = 1.0 + a * lam - lam * lam
    x = np.linspace(0.0, max(mu, 0.0) + 12.0, 2_000_001)
    pdf = np.exp(-0.5 * (x - mu) ** 2) / math.sqrt(2.0 * math.pi) / tail
    trapezoid = getattr(np, "trapezoid", None) or np.trapz
    m4 = float(trapezoid((x - mean) ** 4 * pdf, x))
    return mean, var, m4


# ---- data: the fixtures' inputs, thresholded --------------------------------------------------
def _open(path):
    return gzip.open(path, "rt") if path.endswith(".gz") else open(path, "r")


def write_thresholded(src, dst, threshold):
    """Copy a libfm text file (plain or .gz) with target >= threshold -> 1, else -1: the rule of the
    cls_* fixtures, shared with their generator (tests/golden/make_cls_golden.py). Returns the rows."""
    n = 0
    with _open(src) as fi, open(dst, "w") as fo:
        for line in fi:
            if not line.strip():
                continue
            y, _, rest = line.partition(" ")
            fo.write(("1" if float(y) >= threshold else "-1") + (" " + rest if rest else "\n"))
            n += 1
    return n


def case_files(tmpdir, data, threshold):
    d = os.path.join(GOLDEN, data)
    ext = ".libfm.gz" if data == "sa_split" else ".libfm"
    out = {}
    for part in ("train", "test"):
        out[part] = os.path.join(str(tmpdir), "%s_%s.libfm" % (data, part))
        if not os.path.exists(out[part]):
            write_thresholded(os.path.join(d, part + ext), out[part], threshold)
    return out


def load_trace(name):
    with open(os.path.join(GOLDEN, name, "trace.json")) as fh:
        t = json.load(fh)
    t["pred"] = np.load(os.path.join(GOLDEN, name, "pred.npy"))   # the reference's -out file
    return t

"""NumPy restatement of the counter-based generator of VBFM_RNG_DEVICE, written from the keying
documented in include/vbfm.h and csrc/vbfm_class_math.h: the per-attribute normals, the
initialisation of fm.v / fm.w, the keyed truncated normals of task c's row step and the table of
stream ids of a run. Pinned against the header compiled for the host by tests/test_device_rng_cpu.py;
the GPU tests (tests/test_device_rng_gpu.py) hold the kernels to it draw for draw.

  h(seed, stream)        = seed * K1 + stream * K2                        (uint64, wrapping)
  normal(seed, stream, j): u1 = ((splitmix64(h + 2j) >> 11) + 1) * 2^-53, u2 = (splitmix64(h + 2j + 1) >> 11) * 2^-53,
                           sqrt(-2 log u1) * cos(2 pi u2)
  row key                = splitmix64(splitmix64(h) ^ row); uniform i of attempt t = (splitmix64(key + 2t + i) >> 11) * 2^-53
"""
import math

import numpy as np

import class_ref as cr
from synth import K1, K2, splitmix64

CLASS_STREAM = 1 << 63          # | iteration: the row draws of task c
INIT_STREAM = 1 << 62           # | 21: fm.v, | 22: fm.w of the device-mode initialisation
INIT_V, INIT_W = INIT_STREAM | 21, INIT_STREAM | 22
CLASS_MAX_ATTEMPTS = 64
CLASS_OK, CLASS_NONFINITE, CLASS_CAPPED = 0, 1, 2
TWO_PI = 6.283185307179586
_ONE, _E11 = np.uint64(1), np.uint64(11)
# libm's log, cos and exp, element by element: what the header compiled for the host calls, so the
# restatement can be held to it within a few ulp of the result (NumPy's vector forms round differently)
_log = np.vectorize(math.log, otypes=[np.float64])
_cos = np.vectorize(math.cos, otypes=[np.float64])
_exp = np.vectorize(math.exp, otypes=[np.float64])


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def _base(seed, stream):
    with np.errstate(over="ignore"):
        return _u64(int(seed)) * K1 + _u64(int(stream)) * K2


def _unit(x):
    return (x >> _E11).astype(np.float64) * 2.0 ** -53


def device_normal(seed, stream, j):
    """The standard normal at counter j of (seed, stream), vectorised over j."""
    with np.errstate(over="ignore"):
        b = _base(seed, stream) + np.uint64(2) * _u64(j)
        u1 = ((splitmix64(b) >> _E11).astype(np.float64) + 1.0) * 2.0 ** -53
        u2 = _unit(splitmix64(b + _ONE))
    return np.sqrt(-2.0 * _log(u1)) * _cos(TWO_PI * u2)


def attr_stream(it, f, k):
    """Stream of the attribute draws of iteration it (0-based), sweep f (-1: draw_w)."""
    return int(it) * (int(k) + 1) + (0 if f < 0 else int(f) + 1)


def sweep_normals(seed, it, f, k, D):
    return device_normal(seed, attr_stream(it, f, k), np.arange(D, dtype=np.uint64))


def init_params(seed, init_stdev, k, D):
    """fm.w [D] and fm.v [k*D] ([f][j]) of the device-mode initialisation: v_f[j] takes counter
    j * k + f of its stream."""
    w = init_stdev * device_normal(seed, INIT_W, np.arange(D, dtype=np.uint64))
    v = init_stdev * device_normal(seed, INIT_V, np.arange(k * D, dtype=np.uint64))
    return w, v.reshape(D, k).T.copy().reshape(-1)


def stream_table(k, iters):
    """Every stream id a device-mode run of `iters` iterations draws from, as (name, id)."""
    t = [("init v", INIT_V), ("init w", INIT_W)]
    for it in range(iters):
        t += [("iter %d sweep %d" % (it, f), attr_stream(it, f, k)) for f in range(-1, k)]
        t.append(("iter %d rows" % it, CLASS_STREAM | it))
    return t


def row_key(seed, stream, rows):
    with np.errstate(over="ignore"):
        return splitmix64(splitmix64(_base(seed, stream)) ^ _u64(rows))


def key_uniform(key, attempt, i):
    with np.errstate(over="ignore"):
        return _unit(splitmix64(key + np.uint64(2 * attempt + i)))


def left_tgaussian_keyed(left, key, cap=CLASS_MAX_ATTEMPTS):
    """A standard normal truncated to [left, inf) per row on the row's keyed uniforms: Box-Muller
    rejection for left <= 0, Robert's translated exponential above. Returns (accepted, attempts, z,
    dist): dist is the smallest distance of any of the row's accept / reject comparisons from its
    boundary, |z - left| or |u - d|."""
    left = np.asarray(left, dtype=np.float64)
    n = left.shape[0]
    naive = left <= 0.0
    alpha_star = 0.5 * (left + np.sqrt(left * left + 4.0))
    done = np.zeros(n, dtype=bool)
    attempts = np.zeros(n, dtype=np.int64)
    out = np.full(n, np.nan)
    dist = np.full(n, np.inf)
    for t in range(cap):
        act = ~done
        if not act.any():
            break
        a0, a1 = key_uniform(key, t, 0), key_uniform(key, t, 1)
        attempts[act] += 1
        lg = _log(1.0 - a0)
        zn = np.sqrt(-2.0 * lg) * _cos(TWO_PI * a1)
        zr = -lg / alpha_star + left
        d = zr - alpha_star
        d = _exp(-(d * d) / 2)
        z = np.where(naive, zn, zr)
        acc = np.where(naive, ~(zn < left), a1 < d)
        dd = np.where(naive, np.abs(zn - left), np.abs(a1 - d))
        dist = np.where(act, np.minimum(dist, dd), dist)
        new = act & acc
        out[new] = z[new]
        done |= new
    return done, attempts, out, dist


def class_sample_target(yhat, positive, seed, stream, rows, cap=CLASS_MAX_ATTEMPTS):
    """The latent target of task c's row step per row: N(yhat, 1) truncated to [0, inf) for a
    positive row, to (-inf, 0] otherwise. Returns (s, attempts, flag, dist)."""
    yhat = np.asarray(yhat, dtype=np.float64)
    positive = np.asarray(positive, dtype=bool)
    with np.errstate(invalid="ignore"):
        finite = np.abs(yhat) <= np.finfo(np.float64).max
    yh = np.where(finite, yhat, 0.0)
    ok, attempts, z, dist = left_tgaussian_keyed(np.where(positive, -yh, yh), row_key(seed, stream, rows), cap)
    s = np.where(positive, yh + z, yh - z)
    flag = np.full(yhat.shape[0], CLASS_OK, dtype=np.int64)
    capped = finite & ~ok
    if capped.any():
        s[capped] = cr.expect_target(yh[capped], np.where(positive[capped], 1.0, -1.0))
        flag[capped] = CLASS_CAPPED
    s[~finite] = np.nan
    attempts[~finite] = 0
    dist[~finite] = np.inf
    flag[~finite] = CLASS_NONFINITE
    return s, attempts, flag, dist

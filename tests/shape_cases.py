"""What tests/test_shapes_cpu.py and tests/test_shapes_gpu.py share: the five data sets whose levels
run each workgroup shape of dispatch_shape (csrc/vbfm_device.h), the conditions that put a data set
into its shape, and the CPU oracle's chains on them (tests/oracle_ctypes.py), computed once.

Every data set is synth.generate_columns over synth.SHAPE_COLUMNS[shape]: three one-hot fields, so
three dependency levels, each holding columns of CAP, CAP + 1, 2 CAP + 1, 1, CAP - 1 and CAP / 2
entries (CAP = BLOCK x R) around a mean inside the shape's band.
"""
import os

import numpy as np

import oracle_ctypes as oc
import synth

SHAPES = list(synth.SHAPE_COLUMNS)            # (BLOCK, R), in the table's order
SHAPE_IDS = ["%dx%d" % s for s in SHAPES]
ITERS, SEED, INIT_STDEV = 3, 5, 0.1
REGULAR = (0.5, 1.0, 2.0)                     # ALS: -regular r0,rw,rv (without it ALS chains can diverge)
# settings that change the shape table, the segment rule or the layout: unset in every shape test
SHAPE_ENV = ("VBFM_SMALL_MAX", "VBFM_SEG_MIN", "VBFM_SEG_LEN", "VBFM_LONG", "VBFM_LAYOUT")

_cache = {}


def data(shape, xmode=1):
    """(train, test, nf_train, nf_test, D) of the shape's data set; the sets as (row_ptr, feat, val, y)."""
    key = ("data", shape, xmode)
    if key not in _cache:
        tr, te, nf, nft = synth.generate_columns(synth.SHAPE_COLUMNS[shape], 100 + SHAPES.index(shape), xmode)
        _cache[key] = (tr, te, nf, nft, nft + 1)
    return _cache[key]


def check_conditions(shape, level, num_levels, col_ptr):
    """What puts the data set into `shape`, asserted from a schedule (one level per feature,
    1-based) and the train CSC's col_ptr: the settings that move the table are unset; every level's
    mean column length lies in the shape's band; no column crosses the segment rule, so the columns
    beyond CAP are streamed whole; and the level holds the edges CAP, CAP + 1 and 2 CAP + 1."""
    for name in SHAPE_ENV:
        assert name not in os.environ, name
    assert num_levels == 3
    block, r = shape
    cap = block * r
    lens = np.diff(np.asarray(col_ptr).astype(np.int64))
    for l, (mean, longest) in enumerate(synth.level_means(level, num_levels, col_ptr), 1):
        assert synth.shape_of_mean(mean) == shape, "level %d: mean column %d runs %r, not %r" % (
            l, mean, synth.shape_of_mean(mean), shape)
        assert longest <= max(synth.SEG_MIN, synth.SEG_MEANS * mean), "level %d: a column of %d is segmented" % (
            l, longest)
        have = set(lens[np.asarray(level) == l].tolist())
        assert {1, cap // 2, cap - 1, cap, cap + 1, 2 * cap + 1} <= have, (l, sorted(have))


def _csr(d):
    return len(d[3]), d[0], d[1], d[2], d[3]


def oracle_vb(shape, k, xmode=1):
    """The oracle's VB state after ITERS iterations: rows e, t, q, tq, tz, mu_w, mu_v, free_energy[ITERS]."""
    key = ("vb", shape, k, xmode)
    if key not in _cache:
        tr, te, _, _, D = data(shape, xmode)
        o = oc.VB(1, 1, k, D)
        o.init_params(SEED, INIT_STDEV)
        o.attach(oc.Data(csr=_csr(tr)), oc.Data(csr=_csr(te)))
        o.init_caches()
        fe = []
        for _ in range(ITERS):
            o.iterate()
            fe.append(o.s.last_free_energy)
        r, p = o.rows(), o.params()
        _cache[key] = dict(r, mu_w=p["mu_w"], mu_v=p["mu_v"], free_energy=np.asarray(fe))
    return _cache[key]


def oracle_mc(shape, method, k, xmode=1):
    """The oracle's ALS (-regular REGULAR) or MCMC chain: ([(rmse_all, rmse_this, train_rmse)] per
    iteration, final parameters)."""
    key = (method, shape, k, xmode)
    if key not in _cache:
        tr, te, _, _, D = data(shape, xmode)
        reg = REGULAR if method == "als" else (0.0, 0.0, 0.0)
        o = oc.ALS(1, 1, k, D, method=method, reg0=reg[0])
        o.init_params(SEED, INIT_STDEV)
        o.set_lambda(np.full(1, reg[1]), np.full(k, reg[2]))
        o.attach(oc.Data(csr=_csr(tr)), oc.Data(csr=_csr(te)))
        trace = [o.iterate() for _ in range(ITERS)]
        _cache[key] = (trace, o.params())
    return _cache[key]

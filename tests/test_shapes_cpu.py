"""The data sets of tests/test_shapes_gpu.py land where they are meant to, checked without a GPU.

tests/test_shapes_gpu.py holds every workgroup shape of the level sweeps (dispatch_shape,
csrc/vbfm_device.h) to the CPU oracle on data whose column lengths are prescribed
(synth.generate_columns over synth.SHAPE_COLUMNS). A shape is reached through the level's mean
column length, so a revision of the shape table or of the segment rule can move a data set out of
the shape it is meant to pin without any GPU test failing. These tests restate the table
(synth.SHAPE_TABLE, synth.SEG_MIN / SEG_MEANS) and fail, naming the band, when a list no longer
lands in it: revise the table's restatement and the lists together.
"""
import os
import re

import numpy as np
import pytest

import oracle_ctypes as oc
import shape_cases as sc
import shards
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scalable-variational-bayesian-factorization-machine_amd", "csrc")


@pytest.fixture(autouse=True)
def _no_shape_env(monkeypatch):
    for name in sc.SHAPE_ENV:
        monkeypatch.delenv(name, raising=False)


def test_restated_table_is_the_library_s():
    """synth.SHAPE_TABLE against the text of dispatch_shape and shape_small_max, and the segment
    rule against build_long_segs: the restatement follows the source."""
    with open(os.path.join(CSRC, "vbfm_device.h")) as fh:
        src = fh.read()
    body = src[src.index("inline void dispatch_shape"):]
    body = body[:body.index("\n}")]
    small = int(re.search(r'return e \? \(uint32_t\)atoi\(e\) : (\d+)u;', src).group(1))
    rows = re.findall(r"(?:if|else if) \(avg <= ([\w()]+)\) f\(B(\d+)\(\), R(\d+)\(\)\);", body)
    last = re.search(r"else f\(B(\d+)\(\), R(\d+)\(\)\);", body)
    table = [(small if u == "shape_small_max()" else int(u), int(b), int(r)) for u, b, r in rows]
    table.append((None, int(last.group(1)), int(last.group(2))))
    assert tuple(table) == synth.SHAPE_TABLE
    with open(os.path.join(CSRC, "vbfm_store.hip")) as fh:
        store = fh.read()
    assert "std::max<uint64_t>(%du, std::min<uint64_t>(%d * mean, 1u << 30))" % (synth.SEG_MIN, synth.SEG_MEANS) in store


def test_every_shape_has_a_list():
    assert sorted(sc.SHAPES) == sorted((b, r) for _, b, r in synth.SHAPE_TABLE)


@pytest.mark.parametrize("xmode", [1, 0])
@pytest.mark.parametrize("shape", sc.SHAPES, ids=sc.SHAPE_IDS)
def test_lists_land_in_their_bands(shape, xmode):
    """Every level of the shape's data set has its mean column length in the shape's band, no
    column beyond the segment rule, and the edges CAP, CAP + 1, 2 CAP + 1, 1, CAP - 1, CAP / 2."""
    tr, te, nf, nft, D = sc.data(shape, xmode)
    rp, feat, val, y = tr
    lengths = synth.SHAPE_COLUMNS[shape]
    assert len(y) == sum(lengths) <= 5634
    lv = shards.levels(rp.astype(np.int64), feat.astype(np.int64), nf)
    col_ptr, crow, cval = synth.csr_to_csc(len(y), nf, rp, feat, val)
    sc.check_conditions(shape, lv, int(lv.max()), col_ptr)
    m = len(lengths)
    cols = np.diff(col_ptr.astype(np.int64)).reshape(3, m)
    for f in range(3):                       # the list, rotated per field
        assert cols[f].tolist() == [lengths[(c + f) % m] for c in range(m)]
    fe = feat.reshape(-1, 3).astype(np.int64)
    for f in range(1, 3):                    # no field is a copy of another
        assert not np.array_equal(fe[:, f] - f * m, fe[:, 0])
    assert (val == 1).all() if xmode == 0 else (val.min() >= 0.5 and val.max() < 1.5 and (val != 1).any())
    # the test set stays on the train ids, but for one attribute that no train row has
    assert te[1].max() == nf == nft - 1 and int((te[1] == nf).sum()) == 1
    assert len(np.unique(y)) > 2


def test_a_moved_threshold_is_noticed(monkeypatch):
    """The check itself: with the 64 x 2 band's edge moved below its list's mean, the list is
    reported out of its band."""
    monkeypatch.setattr(synth, "SHAPE_TABLE", ((100, 64, 2),) + synth.SHAPE_TABLE[1:])
    tr, _, nf, _, _ = sc.data((64, 2))
    lv = shards.levels(tr[0].astype(np.int64), tr[1].astype(np.int64), nf)
    col_ptr, _, _ = synth.csr_to_csc(len(tr[3]), nf, tr[0], tr[1], tr[2])
    with pytest.raises(AssertionError, match="mean column 117"):
        sc.check_conditions((64, 2), lv, 3, col_ptr)


@pytest.mark.parametrize("shape", sc.SHAPES, ids=sc.SHAPE_IDS)
def test_a_lost_record_is_far_beyond_the_bounds(shape):
    """What the GPU tests' bounds (1e-12 for VB, 1e-9 for ALS / MCMC) can see: with the x of one
    record zeroed -- the last entry of a level's 2 CAP + 1 column, the tail a chunked sweep could
    lose -- the oracle's own results move by far more. One record of n carries about 1 / n of its
    column's statistics, n <= 2,049: the parameters must move by at least 1e-6, a thousand times
    the wider bound, in every level and for every learner."""
    tr, te, nf, _, D = sc.data(shape)
    rp, feat, val, y = tr
    cap, m = shape[0] * shape[1], len(synth.SHAPE_COLUMNS[shape])
    test = oc.Data(csr=(len(te[3]),) + te)
    for f in range(3):
        fe = feat.reshape(-1, 3)[:, f]
        j = int(np.flatnonzero(np.bincount(fe, minlength=nf)[f * m:(f + 1) * m] == 2 * cap + 1)[0]) + f * m
        v2 = val.copy()
        v2[int(np.flatnonzero(fe == j)[-1]) * 3 + f] = 0.0
        o = oc.VB(1, 1, 3, D)
        o.init_params(sc.SEED, sc.INIT_STDEV)
        o.attach(oc.Data(csr=(len(y), rp, feat, v2, y)), test)
        o.init_caches()
        for _ in range(sc.ITERS):
            o.iterate()
        ref = sc.oracle_vb(shape, 3)
        moved = {"vb": np.max(np.abs(o.params()["mu_w"] - ref["mu_w"])) / np.max(np.abs(ref["mu_w"]))}
        for method in ("als", "mcmc"):
            reg = sc.REGULAR if method == "als" else (0.0, 0.0, 0.0)
            a = oc.ALS(1, 1, 3, D, method=method, reg0=reg[0])
            a.init_params(sc.SEED, sc.INIT_STDEV)
            a.set_lambda(np.full(1, reg[1]), np.full(3, reg[2]))
            a.attach(oc.Data(csr=(len(y), rp, feat, v2, y)), test)
            for _ in range(sc.ITERS):
                a.iterate()
            w = sc.oracle_mc(shape, method, 3)[1]["w"]
            moved[method] = np.max(np.abs(a.params()["w"] - w)) / np.max(np.abs(w))
        print(shape, "level", f + 1, moved)
        assert min(moved.values()) >= 1e-6, (f, moved)


@pytest.mark.parametrize("shape", sc.SHAPES, ids=sc.SHAPE_IDS)
def test_oracle_chains_are_finite(shape):
    """The reference side of the GPU tests: three iterations of VB, ALS and MCMC are finite on
    every data set, for every k and x mode the GPU tests compare."""
    for k, xmode in ((3, 1), (2, 1), (0, 1), (3, 0)):
        ref = sc.oracle_vb(shape, k, xmode)
        for key, v in ref.items():
            assert np.isfinite(v).all(), ("vb", k, xmode, key)
        for method in ("als", "mcmc"):
            trace, p = sc.oracle_mc(shape, method, k, xmode)
            assert np.isfinite(np.asarray(trace)).all(), (method, k, xmode, trace)
            assert all(0.1 < t[2] < 3.0 for t in trace), (method, k, xmode, trace)
            for key, v in p.items():
                assert np.isfinite(v).all(), (method, k, xmode, key)

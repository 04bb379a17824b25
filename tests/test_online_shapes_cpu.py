"""The data sets of tests/test_online_shapes_gpu.py land where they are meant to, checked without a GPU.

tests/test_online_shapes_gpu.py holds every lane-group width G of the online learner to the CPU
oracle. G is reached through a level's floor(mean column length) / num_batch (ov_level and ov_lord_g,
csrc/vbfm_online.hip), and the padded layout through OV_CAP, so a revision of either table or of
OV_CAP can move a data set out of the width it is meant to pin without any GPU test failing. These
tests restate the tables (synth.OV_G_TABLE, synth.OV_LORD_G_TABLE, synth.OV_CAP) and fail, naming the
set and the band, when a list no longer lands in it: revise the restatement and the lists together.

With two batches the batch columns depend on the reference's shuffle, which the oracle draws
(OrOVB.shuffle): the conditions on them are asserted for every epoch and every k the GPU tests run
(the initial draws, so the shuffle, depend on k). If a data seed fails them, change the seed
(online_cases.DATA_SEED), never the condition.
"""
import os
import re

import numpy as np
import pytest

import online_cases as ocs
import oracle_ctypes as oc
import shards
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scalable-variational-bayesian-factorization-machine_amd", "csrc")
CASES = [(name, nb) for name in ocs.SETS for nb in (1, 2) if not (name == "wide" and nb == 2)]
CASE_IDS = ["%s-b%d" % c for c in CASES]

_sched = {}


def schedule(name, nb):
    """(level per train feature, col_ptr, rows of the CSC entries) of the set."""
    if (name, nb) not in _sched:
        tr, _, nf, _, _ = ocs.data(name, nb)
        rp, feat, val, y = tr
        lv = shards.levels(rp.astype(np.int64), feat.astype(np.int64), nf)
        col_ptr, crow, _ = synth.csr_to_csc(len(y), nf, rp, feat, val)
        _sched[name, nb] = (lv, col_ptr, crow)
    return _sched[name, nb]


def test_restated_tables_are_the_library_s():
    """synth.OV_LORD_G_TABLE against the text of ov_lord_g, synth.OV_G_TABLE against ov_level's,
    synth.OV_CAP against OV_CAP: the restatement follows the source."""
    with open(os.path.join(CSRC, "vbfm_online.hip")) as fh:
        src = fh.read()
    body = src[src.index("uint32_t ov_lord_g(uint32_t m)\n{"):]
    body = body[:body.index("\n}")]
    rows = [(int(u), int(g)) for u, g in re.findall(r"m <= (\d+) \? (\d+) :", body)]
    rows.append((None, int(re.search(r": (\d+);", body).group(1))))
    assert tuple(rows) == synth.OV_LORD_G_TABLE
    body = src[src.index("hipError_t ov_level(const LevelArgs &a"):]
    body = body[:body.index("\n}")]
    rows = [(int(u), int(g)) for u, g in re.findall(r"if \(m <= (\d+)\) return launch_ov<(\d+)>", body)]
    rows.append((None, int(re.search(r"\n\treturn launch_ov<(\d+)>", body).group(1))))
    assert tuple(rows) == synth.OV_G_TABLE
    assert int(re.search(r"constexpr uint32_t OV_CAP = (\d+);", src).group(1)) == synth.OV_CAP
    # ov_lord_level launches what ov_lord_g says, G <= 64 only
    assert sorted({g for _, g in synth.OV_LORD_G_TABLE}) == sorted(
        int(g) for g in re.findall(r"return launch_ov_lord<(\d+)>", src))


def test_every_width_has_a_set():
    assert sorted(ocs.WIDTHS) == sorted(g for _, g in synth.OV_LORD_G_TABLE)
    assert sorted({ocs.column_g(name) for name in ocs.SETS}) == sorted(g for _, g in synth.OV_G_TABLE)
    for g, lst in synth.ONLINE_COLUMNS.items():
        assert sorted(lst) == [1, g - 1, g, g + 1, 2 * g, 2 * g + 1, 3 * g + 1]


@pytest.mark.parametrize("xmode", [1, 0])
@pytest.mark.parametrize("name,nb", CASES, ids=CASE_IDS)
def test_sets_land_in_their_bands(name, nb, xmode):
    """Every level's floor(mean) / num_batch in the band of G for both tables, the edge lengths in
    every level, a full and a partial workgroup, no feature twice in a row, and with one batch every
    workgroup run of the later levels within OV_CAP (the wide set: beyond it)."""
    tr, te, nf, nft, D = ocs.data(name, nb, xmode)
    rp, feat, val, y = tr
    lst = ocs.lengths(name, nb)
    assert 200 <= len(y) == sum(lst) <= 3000
    lv, col_ptr, crow = schedule(name, nb)
    ocs.check_conditions(name, nb, lv, int(lv.max()), col_ptr, crow)
    m = len(lst)
    cols = np.diff(col_ptr.astype(np.int64)).reshape(3, m)
    for f in range(3):                       # the list, rotated per field
        assert cols[f].tolist() == [lst[(c + f) % m] for c in range(m)]
        assert (lv.reshape(3, m)[f] == f + 1).all()
    fe = np.sort(feat.reshape(-1, 3).astype(np.int64), axis=1)
    assert (np.diff(fe, axis=1) > 0).all()   # no row lists a feature twice
    assert (val == 1).all() if xmode == 0 else (val.min() >= 0.5 and val.max() < 1.5 and (val != 1).any())
    assert te[1].max() == nf == nft - 1 and int((te[1] == nf).sum()) == 1
    assert len(np.unique(y)) > 2
    if nb == 2:
        assert int((cols == 1).sum()) == 3   # one column per level is absent from one batch


@pytest.mark.parametrize("k", [3, 2, 1, 0])
@pytest.mark.parametrize("name", ocs.SETS[:-1])
def test_batches_keep_their_widths(name, k):
    """Two batches, from the oracle's shuffle after each epoch: every workgroup run of the later
    levels stays within OV_CAP in both batches (the padded layout holds), every level has a batch
    column longer than 2 G (the loop arm runs) and the column of length 1 is empty in one batch."""
    g = ocs.lord_g(name)
    lv, col_ptr, _ = schedule(name, 2)
    full = np.diff(col_ptr.astype(np.int64))
    _, _, bat = ocs.oracle_run(name, 2, k)
    assert len(bat) == ocs.ITERS
    for it, batch in enumerate(bat):
        n = len(batch)
        assert np.bincount(batch, minlength=2).tolist() == [-(-n // 2), n // 2]
        lens = ocs.batch_lengths(name, 2, batch)
        assert (lens.sum(axis=0) == full).all()
        for b in range(2):
            for l in (1, 2, 3):
                assert lens[b][lv == l].max() > 2 * g, (name, k, it, b, l, int(lens[b][lv == l].max()))
                assert lens[b][lv == l].sum() == lens[b].sum() // 3
            for l in (2, 3):
                r = max(ocs.runs(name, lv, l, None, lens[b]))
                assert r <= synth.OV_CAP, "%s k=%d epoch %d batch %d level %d: a run of %d records" % (
                    name, k, it, b, l, r)
        assert sorted(lens[:, full == 1].min(axis=0).tolist()) == [0, 0, 0]


@pytest.mark.parametrize("table", ["OV_LORD_G_TABLE", "OV_G_TABLE"])
def test_a_moved_threshold_is_noticed(table, monkeypatch):
    """The check itself: with the upper edge of the G = 16 band of either table moved below the
    G = 16 list's mean (23 -> 22), the set is reported out of its band, by name."""
    kept = getattr(synth, table)
    monkeypatch.setattr(synth, table, tuple((22, g) if upto == 24 else (upto, g) for upto, g in kept))
    lv, col_ptr, _ = schedule("g16", 1)
    with pytest.raises(AssertionError, match=r"g16 nb=1 level 1: batch mean column 23 runs G = 32 of %s, "
                       r"not 16 \(band \(13, 22\)\)" % {"OV_LORD_G_TABLE": "ov_lord_g", "OV_G_TABLE": "ov_level"}[table]):
        ocs.check_conditions("g16", 1, lv, 3, col_ptr)
    monkeypatch.setattr(synth, table, kept)
    monkeypatch.setattr(synth, "OV_CAP", 386)       # and a smaller slot: a G = 64 run of level 3 leaves it
    lv, col_ptr, _ = schedule("g64", 1)
    with pytest.raises(AssertionError, match="g64: a workgroup run of 387 records leaves the padded layout"):
        ocs.check_conditions("g64", 1, lv, 3, col_ptr)


@pytest.mark.parametrize("name", ocs.SETS)
def test_a_lost_record_is_far_beyond_the_bound(name):
    """What REL = 1e-9 of the GPU tests can see: with the x of one record zeroed -- the last entry of
    each level's longest column (3 G + 1 entries; 520 in the wide set), the one a lane group's loop or
    a run's tail beyond OV_CAP could lose -- the oracle's own parameters after ITERS epochs of one
    batch move by at least 1e-6, a thousand times the bound, in every level."""
    tr, te, nf, _, D = ocs.data(name, 1)
    rp, feat, val, y = tr
    test = oc.Data(csr=(len(te[3]),) + te)
    _, ref, _ = ocs.oracle_run(name, 1, 3)
    longest = max(ocs.lengths(name, 1))
    m = nf // 3
    for f in range(3):
        fe = feat.reshape(-1, 3)[:, f]
        j = int(np.flatnonzero(np.bincount(fe, minlength=nf)[f * m:(f + 1) * m] == longest)[0]) + f * m
        v2 = val.copy()
        v2[int(np.flatnonzero(fe == j)[-1]) * 3 + f] = 0.0
        o = oc.OVB(1, 1, 3, D, 1)
        o.init(ocs.SEED, ocs.INIT_STDEV, oc.Data(csr=(len(y), rp, feat, v2, y)), test)
        for _ in range(ocs.ITERS):
            o.epoch()
        p = o.params()
        moved = {key: float(np.max(np.abs(p[key] - ref[key])) / np.max(np.abs(ref[key])))
                 for key in ("mu_w", "mu_v", "nat_mu_w", "nat_mu_v")}
        print(name, "level", f + 1, moved)
        assert min(moved.values()) >= 1e-6, (f, moved)


@pytest.mark.parametrize("name,nb", CASES, ids=CASE_IDS)
def test_oracle_runs_are_finite(name, nb):
    """The reference side of the GPU tests: ITERS epochs are finite on every set, for every k, x
    mode and grouping the GPU tests compare."""
    runs = [(3, 1, False), (3, 0, False)]
    if name != "wide":
        runs += [(2, 1, False), (1, 1, False), (0, 1, False)]
    if name in ("g16", "g64"):
        runs.append((3, 1, True))
    for k, xmode, grouped in runs:
        out, p, _ = ocs.oracle_run(name, nb, k, xmode, grouped)
        assert np.isfinite(np.asarray(out)[:, :3 if nb == 1 else 4]).all(), (k, xmode, grouped, out)
        assert all(0.1 < e[0] < 3.0 for e in out), (k, xmode, grouped, out)
        for key, v in p.items():
            assert np.isfinite(v).all(), (k, xmode, grouped, key)

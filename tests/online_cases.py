"""What tests/test_online_shapes_cpu.py and tests/test_online_shapes_gpu.py share: the data sets whose
levels run each lane-group width of the online learner (ov_level and ov_lord_g, csrc/vbfm_online.hip;
restated as synth.OV_G_TABLE / OV_LORD_G_TABLE), the conditions that put a data set into its width,
and the CPU oracle's runs on them (oracle_ctypes.OVB), computed once per process.

Every data set is synth.generate_columns: three one-hot fields, so three dependency levels that hold
every row once -- the per-batch level-ordered store and its padded layout apply.

  ("g<G>", 1)  synth.ONLINE_COLUMNS[G] repeated synth.ONLINE_REPEATS[G] times, one batch: a batch
               column is the whole column, so every level holds columns of exactly 1, G - 1, G,
               G + 1, 2 G, 2 G + 1 and 3 G + 1 entries.
  ("g<G>", 2)  the same list with every length doubled, but for one column that keeps length 1 (empty
               in one of the two batches of every epoch): floor(mean) / 2 stays in G's band. Which
               rows a batch holds comes from the reference's shuffle, so the batch columns scatter
               around the list; batches(...) reads them from the oracle.
  ("wide", 1)  synth.ONLINE_WIDE: the 256-lane column kernel, and k_ov_lord<64> on runs beyond OV_CAP.
"""
import numpy as np

import oracle_ctypes as oc
import synth

WIDTHS = tuple(synth.ONLINE_COLUMNS)               # 4, 8, 16, 32, 64
SETS = ["g%d" % g for g in WIDTHS] + ["wide"]
ITERS, SEED, INIT_STDEV = 3, 5, 0.1                # as tests/shape_cases.py
# what selects a form of the learner: cleared before every run
ONLINE_ENV = ("VBFM_LAYOUT", "VBFM_OV_PAD", "VBFM_OV_FAST", "VBFM_OV_LEGACY")
DATA_SEED = {"g4": 204, "g8": 208, "g16": 216, "g32": 232, "g64": 264, "wide": 300}

_cache = {}


def lord_g(name):
    """Lanes per column of k_ov_lord on the set."""
    return 64 if name == "wide" else int(name[1:])


def column_g(name):
    """Lanes per column of k_ov_{w,v}_level on the set."""
    return 256 if name == "wide" else int(name[1:])


def lengths(name, nb):
    """The column-length list of every field (generate_columns rotates it per field)."""
    if name == "wide":
        assert nb == 1
        return list(synth.ONLINE_WIDE)
    g = lord_g(name)
    out = list(synth.ONLINE_COLUMNS[g]) * synth.ONLINE_REPEATS[g]
    if nb == 1:
        return out
    assert nb == 2
    out = [2 * x for x in out]
    out[out.index(2)] = 1
    return out


def edges(name, nb):
    """The column lengths every level must hold."""
    if name == "wide":
        return set(synth.ONLINE_WIDE)
    e = set(synth.ONLINE_COLUMNS[lord_g(name)])
    return e if nb == 1 else {2 * x for x in e} | {1}


def data(name, nb, xmode=1):
    """(train, test, nf_train, nf_test, D) of the set; train and test as (row_ptr, feat, val, y)."""
    key = ("data", name, nb, xmode)
    if key not in _cache:
        tr, te, nf, nft = synth.generate_columns(lengths(name, nb), DATA_SEED[name] + nb, xmode)
        _cache[key] = (tr, te, nf, nft, nft + 1)
    return _cache[key]


def field_groups(name, nb):
    """One attribute group per field; the attribute no train row has joins the last field's."""
    _, _, nf, _, D = data(name, nb)
    return np.minimum(np.arange(D, dtype=np.uint32) // np.uint32(nf // 3), np.uint32(2))


def runs(name, level, l, col_ptr, lens=None):
    """Records of every k_ov_lord workgroup run of level l (1-based): 256 / G consecutive columns
    of the level, in ascending feature id. `lens`: the columns' lengths if not col_ptr's (a batch)."""
    if lens is None:
        lens = np.diff(np.asarray(col_ptr).astype(np.int64))
    m = np.asarray(lens)[np.asarray(level) == l]
    cpw = 256 // lord_g(name)
    return [int(m[i:i + cpw].sum()) for i in range(0, len(m), cpw)]


def check_conditions(name, nb, level, num_levels, col_ptr, col_rows=None):
    """What puts the set into its width, asserted from a schedule (one level per feature, 1-based)
    and the train CSC: three levels; every level's floor(mean column length) / num_batch in the band
    of G for ov_lord_g and for ov_level; the edge lengths in every level; more than one workgroup
    and a partial last one; no row twice in a column (col_rows given); with one batch, every
    workgroup run of the levels past the first within OV_CAP -- or, the wide set, one beyond it."""
    assert num_levels == 3
    level = np.asarray(level)
    lens = np.diff(np.asarray(col_ptr).astype(np.int64))
    want = edges(name, nb)
    cpw = 256 // lord_g(name)
    for l, (mean, _) in enumerate(synth.level_means(level, num_levels, col_ptr), 1):
        avg = mean // nb
        for what, table, g in (("ov_lord_g", synth.OV_LORD_G_TABLE, lord_g(name)),
                               ("ov_level", synth.OV_G_TABLE, column_g(name))):
            got = synth.ov_g_of(avg, table)
            assert got == g, "%s nb=%d level %d: batch mean column %d runs G = %d of %s, not %d (band %r)" % (
                name, nb, l, avg, got, what, g, synth.ov_band(g, table))
        have = set(lens[level == l].tolist())
        assert want <= have, (name, nb, l, sorted(want - have))
        ncol = int((level == l).sum())
        assert ncol > cpw and ncol % cpw != 0, (name, l, ncol, cpw)
    if col_rows is not None:
        col = np.repeat(np.arange(len(lens)), lens)
        pair = col.astype(np.int64) * (int(np.max(col_rows)) + 1) + np.asarray(col_rows).astype(np.int64)
        assert len(np.unique(pair)) == len(pair), "a row lists a feature twice"
    if nb == 1:
        longest = max(max(runs(name, level, l, col_ptr)) for l in (2, 3))
        if name == "wide":
            assert longest > synth.OV_CAP and lens.max() > synth.OV_CAP, (name, longest)
        else:
            assert longest <= synth.OV_CAP, "%s: a workgroup run of %d records leaves the padded layout" % (
                name, longest)


def _csr(d):
    return len(d[3]), d[0], d[1], d[2], d[3]


def oracle_run(name, nb, k, xmode=1, grouped=False):
    """The oracle's ITERS epochs on the set: ([(rmse, mae, fe_first, fe_last)] per epoch, its final
    params(), [batch of every train row] per epoch from its shuffle)."""
    key = ("ovb", name, nb, k, xmode, grouped)
    if key not in _cache:
        tr, te, _, _, D = data(name, nb, xmode)
        o = oc.OVB(1, 1, k, D, nb, field_groups(name, nb) if grouped else None)
        train, test = oc.Data(csr=_csr(tr)), oc.Data(csr=_csr(te))
        o.init(SEED, INIT_STDEV, train, test)
        out, bat = [], []
        n = len(tr[3])
        for _ in range(ITERS):
            out.append(o.epoch())
            sh = oc.arr(o.s.shuffle, n, np.uint32).astype(np.int64)
            size = -(-n // nb)
            assert size == o.s.size_except_last
            bat.append(-(-sh // size) - 1)          # ceil(shuffle / size) - 1
        _cache[key] = (out, o.params(), bat)
    return _cache[key]


def batch_lengths(name, nb, batch):
    """[num_batch][nf] column lengths of every batch, from the batch of every train row."""
    tr, _, nf, _, _ = data(name, nb)
    feat = tr[1].astype(np.int64)
    b = np.repeat(np.asarray(batch), 3)
    return np.bincount(b * nf + feat, minlength=nb * nf).reshape(nb, nf)

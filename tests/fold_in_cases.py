"""The models and support rows of tests/test_fold_in_gpu.py, and the restated width table of
vbfm_fold_in (csrc/vbfm_fold_plan.h: FOLD_R, FOLD_WG, FOLD_WG_LDS_ROWS, fold_auto_width).

A case is one call: a synthetic VB model of D = 40 attributes and, for a lane width G, nine new
attributes whose columns hold 0, 1, G - 1, G, G + 1, 2G + 1, G*R, G*R + 1 and 3*G*R + 1 rows -- for
G = 256 (one workgroup per column) "G*R" is the FOLD_WG_LDS_ROWS rows that path keeps in LDS. Rows
hold 0 to 3 frozen entries (a repeated frozen id among them, and rows with the new entry alone), the
new entry at a varying position with x != 1, and the columns' rows are interleaved."""
import numpy as np

FOLD_R = 4
FOLD_WG = 256
FOLD_WG_LDS_ROWS = 4096
WIDTHS = (4, 8, 16, 32, 64, FOLD_WG)
KS = (0, 1, 3, 8, 64, 65, 100)
D = 40
PRIOR_IDS = (10, 30)     # the sub-range of the derived priors
# (upper bound of the mean rows per non-empty column, width); beyond the last: FOLD_WG
AUTO_TABLE = ((8, 4), (16, 8), (32, 16), (64, 32), (256, 64))


def group_rows(G):
    """The rows up to which a column stays on its first path at width G."""
    return FOLD_WG_LDS_ROWS if G == FOLD_WG else G * FOLD_R


def column_lengths(G):
    gr = group_rows(G)
    return [0, 1, G - 1, G, G + 1, 2 * G + 1, gr, gr + 1, 3 * gr + 1]


def path(G, length):
    """The kernel and the home of e for a column of `length` rows at width G."""
    if G != FOLD_WG and length <= G * FOLD_R:
        return "group"
    return "wg_lds" if length <= FOLD_WG_LDS_ROWS else "wg_mem"


# what every column of column_lengths(G) is meant to pin
EXPECTED_PATHS = {G: ["group"] * 7 + ["wg_lds", "wg_lds"] for G in WIDTHS if G != FOLD_WG}
EXPECTED_PATHS[FOLD_WG] = ["wg_lds"] * 7 + ["wg_mem", "wg_mem"]


def auto_width(rows, with_rows):
    mean = rows / with_rows if with_rows else 0.0
    for upper, g in AUTO_TABLE:
        if mean <= upper:
            return g
    return FOLD_WG


def model(k, k0, k1, seed=0, d=D):
    """A synthetic VB model as Model.write_params takes it: (info, params)."""
    rng = np.random.default_rng(1000 + 17 * k + seed)
    info = dict(kind=0, k0=k0, k1=k1, num_factor=k, num_attribute=d, min_target=-5.0, max_target=5.0, iter=7,
                has_variance=1, w0_or_mu0=0.5, sigma_0_dash=0.02, alpha=2.0)
    scale = 0.6 / np.sqrt(max(k, 1))
    p = dict(mu_w=0.3 * rng.standard_normal(d), sigma_w=0.01 + 0.05 * rng.random(d),
             mu_v=scale * rng.standard_normal(k * d), sigma_v=(0.01 + 0.05 * rng.random(k * d)) * scale * scale,
             mu_0_dash=0.5, sigma_0_dash=0.02, alpha=2.0)
    p["info"] = dict(info)
    return info, p


def columns(lengths, seed, d=D):
    """Per new attribute the rows in their order: a list (one per column) of lists of (ids, x, y) with
    the new entry (id d + c) somewhere inside."""
    rng = np.random.default_rng(seed)
    cols = []
    for c, n in enumerate(lengths):
        rows = []
        for i in range(n):
            nf = (i + c) % 4
            ids = list(rng.integers(0, d, size=nf))
            if nf == 3 and i % 8 == 3:
                ids[1] = ids[0]                       # a repeated frozen id
            xs = list((0.25 + rng.random(nf)).astype(np.float32))
            at = int(rng.integers(0, nf + 1))
            ids.insert(at, d + c)
            xs.insert(at, np.float32(0.5 + rng.random()))
            rows.append((ids, xs, np.float32(rng.standard_normal())))
        cols.append(rows)
    return cols


def interleave(cols, seed):
    """The columns' rows merged in a random order that keeps every column's own order: ((row_ptr, feat,
    val), target, col_of_row, index_in_col)."""
    rng = np.random.default_rng(seed)
    labels = np.concatenate([np.full(len(rows), c, dtype=np.int64) for c, rows in enumerate(cols)] + [np.zeros(0, dtype=np.int64)])
    labels = labels[rng.permutation(len(labels))]
    nxt = [0] * len(cols)
    rp, feat, val, y, idx = [0], [], [], [], []
    for c in labels:
        ids, xs, t = cols[c][nxt[c]]
        idx.append(nxt[c])
        nxt[c] += 1
        feat.extend(ids)
        val.extend(xs)
        y.append(t)
        rp.append(len(feat))
    rows = (np.asarray(rp, dtype=np.uint64), np.asarray(feat, dtype=np.uint32), np.asarray(val, dtype=np.float32))
    return rows, np.asarray(y, dtype=np.float32), labels, np.asarray(idx, dtype=np.int64)


def variants(G, k):
    """The (k1, k0, priors) of the calls of one (G, k): both k1, both k0, and given as well as derived
    priors (the latter over PRIOR_IDS) for either k1 and either k0."""
    out = []
    for k1 in (0, 1):
        for k0 in (0, 1):
            given = (k1 + k0) % 2 == 0
            rng = np.random.default_rng(G + k + 2 * k1 + k0)
            pri = dict(prior_w=float(0.5 + rng.random()), prior_v=0.5 + 4 * rng.random(k)) if given else dict(prior_ids=PRIOR_IDS)
            out.append((k1, k0, pri))
    return out


# ---- the held-out users of tests/test_fold_in_gpu.py::test_fold_in_beats_skipping ------------------------
HELD_F, HELD_S, HELD_ROWS, HELD_K, HELD_USERS = 3, 40, 4000, 2, 10


def heldout_set():
    """A planted-model set of synth.generate (3 fields x 40 ids, 4,000 rows, x != 1) with field 0 as the
    users, ids renumbered so that the users come last and the 10 held-out ones beyond the model's
    D = 110: (D, (lo, hi) of the user block, train, support, test), each ((row_ptr, feat, val), y).
    train holds the rows of the kept users; support and test are alternate rows of the held-out ones."""
    import synth
    F, S, N = HELD_F, HELD_S, HELD_ROWS
    _, feat, val, y = synth.generate(N, F, S, 21, 1)
    fe = feat.reshape(N, F).astype(np.int64)
    ids = np.stack([2 * S + fe[:, 0], fe[:, 1] - S, fe[:, 2] - S], axis=1)
    D = 3 * S - HELD_USERS
    held = fe[:, 0] >= S - HELD_USERS
    order = np.argsort(ids, axis=1, kind="stable")
    ids, xs = np.take_along_axis(ids, order, 1), np.take_along_axis(val.reshape(N, F), order, 1)

    def part(mask):
        n = int(mask.sum())
        return (np.arange(n + 1, dtype=np.uint64) * np.uint64(F), ids[mask].ravel().astype(np.uint32),
                xs[mask].ravel().astype(np.float32)), y[mask]

    rows_held = np.nonzero(held)[0]
    sup, tst = np.zeros(N, dtype=bool), np.zeros(N, dtype=bool)
    sup[rows_held[0::2]] = True
    tst[rows_held[1::2]] = True
    return D, (2 * S, D), part(~held), part(sup), part(tst)


def heldout_model(D, train, iters=15):
    """The VB parameters of the C oracle after `iters` iterations on train: (info, params)."""
    import oracle_ctypes as oc
    (rp, feat, val), y = train
    o = oc.VB(1, 1, HELD_K, D)
    o.init_params(5, 0.1)
    d = oc.Data(csr=(len(y), rp, feat, val, y))
    o.attach(d, d)
    o.init_caches()
    for _ in range(iters):
        o.iterate()
    p = o.params()
    alpha, _, mu0, s0d = (float(v) for v in p["scalars"])
    info = dict(kind=0, k0=1, k1=1, num_factor=HELD_K, num_attribute=D, min_target=1.0, max_target=5.0, iter=iters,
                has_variance=1, w0_or_mu0=mu0, sigma_0_dash=s0d, alpha=alpha)
    params = dict(mu_w=p["mu_w"].copy(), sigma_w=p["sigma_w"].copy(), mu_v=p["mu_v"].copy(), sigma_v=p["sigma_v"].copy(),
                  mu_0_dash=mu0, sigma_0_dash=s0d, alpha=alpha, info=dict(info))
    return info, params

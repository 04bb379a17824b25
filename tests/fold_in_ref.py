"""NumPy restatement of include/vbfm.h "fold-in": the frozen sums of a support row in ascending id,
the sweep over a new attribute's rows in row order in float64 with the reference's guards
(fm_learn_vb.h:545-565, :600-619), tol, the derived priors (:474-498), and the exact fixed point the
sweep converges to. No GPU and no library: plain arrays in, plain arrays out.

A model is a dict as vbfm.Model.read_params returns it (mu_w, sigma_w [D]; mu_v, sigma_v [k*D] as
[f][j]; mu_0_dash, alpha) with info = {k0, k1, num_factor, num_attribute}; support rows are
(row_ptr, feat, val) with float32 values and a float32 target."""
import numpy as np


def seq_sum(a):
    """The sum of a in index order (np.sum adds pairwise)."""
    return float(np.cumsum(a)[-1]) if len(a) else 0.0


def split_rows(D, row_ptr, feat, val):
    """Per row: the new id, its value, and the frozen entries in ascending id (entries of one id in
    the order given). Raises ValueError naming the first row that does not hold exactly one new id."""
    n = len(row_ptr) - 1
    new_id, new_x, frozen = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.float32), []
    for r in range(n):
        b, e = int(row_ptr[r]), int(row_ptr[r + 1])
        ids, xs = np.asarray(feat[b:e], dtype=np.int64), np.asarray(val[b:e], dtype=np.float32)
        new = np.nonzero(ids >= D)[0]
        if len(new) != 1:
            raise ValueError("row %d holds %d new feature ids" % (r, len(new)))
        new_id[r], new_x[r] = ids[new[0]], xs[new[0]]
        keep = ids < D
        order = np.argsort(ids[keep], kind="stable")
        frozen.append((ids[keep][order], xs[keep][order]))
    return new_id, new_x, frozen


def frozen_sums(model, frozen):
    """base (the unclipped mean, predict_data_and_write_to_eterms, fm_learn_vb.h:70-203), A [n][k] =
    sum mu_v x and B [n][k] = sum sigma_v x^2 of every row's frozen entries."""
    info = model["info"]
    k, D = info["num_factor"], info["num_attribute"]
    mu_v, sg_v = model["mu_v"].reshape(k, D), model["sigma_v"].reshape(k, D)
    n = len(frozen)
    # all rows at once: entry slot l of every row (rows padded with x = 0), the slots added in order
    L = max([len(ids) for ids, _ in frozen], default=0)
    ids, x = np.zeros((n, L), dtype=np.int64), np.zeros((n, L))
    for r, (i, xs) in enumerate(frozen):
        ids[r, :len(i)], x[r, :len(i)] = i, xs
    base, A, B = np.zeros(n), np.zeros((n, k)), np.zeros((n, k))
    e, q = np.zeros(n), np.zeros(n)
    for f in range(k):
        for l in range(L):
            A[:, f] += mu_v[f, ids[:, l]] * x[:, l]
            B[:, f] += sg_v[f, ids[:, l]] * x[:, l] * x[:, l]
        e += 0.5 * A[:, f] * A[:, f]
        for l in range(L):
            q -= 0.5 * mu_v[f, ids[:, l]] * mu_v[f, ids[:, l]] * x[:, l] * x[:, l]
    if info["k1"]:
        for l in range(L):
            q += model["mu_w"][ids[:, l]] * x[:, l]
    base = e + q
    if info["k0"]:
        base = base + model["mu_0_dash"]
    return base, A, B


def derived_priors(model, lo=None, hi=None):
    """lambda_w, lambda_v[f] of the hyper step over the ids [lo, hi) as one group; [0] is 0 with k1 = 0."""
    info = model["info"]
    k, D = info["num_factor"], info["num_attribute"]
    lo, hi = (0, D) if lo is None else (lo, hi)
    n = hi - lo
    lam = np.zeros(1 + k)
    if info["k1"]:
        lam[0] = n / np.sum(model["mu_w"][lo:hi] ** 2 + model["sigma_w"][lo:hi])
    mu_v, sg_v = model["mu_v"].reshape(k, D), model["sigma_v"].reshape(k, D)
    for f in range(k):
        lam[1 + f] = n / np.sum(mu_v[f, lo:hi] ** 2 + sg_v[f, lo:hi])
    return lam


def _update(lam, alpha, S, M, mu, sg):
    """s', the new mean and whether it was taken, with the reference's guards."""
    with np.errstate(all="ignore"):
        s = np.float64(1.0) / np.float64(lam + alpha * S)
        m = s * alpha * np.float64(M)
    if np.isfinite(s):
        sg = float(s)
    if not np.isfinite(m):
        return mu, sg, False
    return float(m), sg, True


def sweep_column(x32, y32, base, A, B, lam, alpha, k1, passes, tol=0.0, on_pass=None):
    """The sweep for one new attribute over its rows in the order given. Returns a dict: w, s_w, v [k],
    s_v [k], e [rows], passes (run), converged, nonfinite. on_pass(passes run, w, v) is called after
    every pass; a true result ends the sweep there."""
    k = A.shape[1]
    x = x32.astype(np.float64)
    with np.errstate(all="ignore"):
        e = y32.astype(np.float64) - base
    w, s_w = 0.0, (1.0 / lam[0] if k1 else 0.0)
    v, s_v = np.zeros(k), 1.0 / lam[1:] if k else np.zeros(0)
    s_v = np.array(s_v, dtype=np.float64)
    out = dict(passes=0, converged=False, nonfinite=0)
    if len(x) == 0:
        return dict(out, w=w, s_w=s_w, v=v, s_v=s_v, e=e)
    for p in range(passes):
        delta = 0.0
        with np.errstate(all="ignore"):
            if k1:
                S, M = seq_sum(x * x), seq_sum(x * (e + x * w))
                wn, s_w, ok = _update(lam[0], alpha, S, M, w, s_w)
                if ok:
                    e = e + x * (w - wn)
                    delta = max(delta, abs(wn - w))
                    w = wn
                else:
                    out["nonfinite"] += 1
            for f in range(k):
                h, h1 = A[:, f], B[:, f]
                S = seq_sum(x * x * h * h + x * x * h1)
                M = seq_sum(x * h * (e + x * v[f] * h))
                vn, s_v[f], ok = _update(lam[1 + f], alpha, S, M, v[f], s_v[f])
                if ok:
                    e = e + x * h * (v[f] - vn)
                    delta = max(delta, abs(vn - v[f]))
                    v[f] = vn
                else:
                    out["nonfinite"] += 1
        out["passes"] = p + 1
        if on_pass is not None and on_pass(p + 1, w, v):
            break
        if tol > 0.0 and delta <= tol:
            out["converged"] = True
            break
    return dict(out, w=w, s_w=s_w, v=v, s_v=s_v, e=e)


def solve_column(x32, y32, base, A, B, lam, alpha, k1):
    """The exact fixed point of the sweep: (diag(lambda_w, lambda_v + alpha sum x^2 B) + alpha Phi'Phi) m =
    alpha Phi'(y - base), Phi = [x, x A]. Returns (w, v)."""
    x = x32.astype(np.float64)
    k = A.shape[1]
    Phi = np.concatenate([x[:, None], x[:, None] * A], axis=1)
    diag = np.concatenate([[lam[0]], lam[1:] + alpha * np.sum(x[:, None] ** 2 * B, axis=0)])
    if not k1:
        Phi, diag = Phi[:, 1:], diag[1:]
    if Phi.shape[1] == 0:
        return 0.0, np.zeros(0)
    m = np.linalg.solve(np.diag(diag) + alpha * Phi.T @ Phi, alpha * Phi.T @ (y32.astype(np.float64) - base))
    return (float(m[0]), m[1:]) if k1 else (0.0, m)


def fold_in(model, rows, target, passes=20, tol=0.0, prior_w=None, prior_v=None, prior_ids=None, num_attribute=None,
            solve=False, split=None):
    """vbfm_fold_in restated. Returns a dict: mu_w, sigma_w [new ids]; mu_v, sigma_v [k][new ids]; resid
    [rows]; prior_used [1 + k]; col_passes [new ids]; stats (the counts of vbfm_fold_stats). solve=True:
    mu_w and mu_v are the exact fixed point instead (sigmas, resid and counts still the sweep's).
    split: split_rows of these rows, where the caller has it already."""
    info = model["info"]
    k, D, k1 = info["num_factor"], info["num_attribute"], info["k1"]
    row_ptr, feat, val = rows
    target = np.asarray(target, dtype=np.float32)
    new_id, new_x, frozen = split if split is not None else split_rows(D, row_ptr, feat, val)
    n = len(new_id)
    D_out = num_attribute if num_attribute else (int(new_id.max()) + 1 if n else D)
    if n and int(new_id.max()) >= D_out:
        raise ValueError("row %d holds feature id beyond num_attribute" % int(np.argmax(new_id >= D_out)))
    lam = derived_priors(model, *(prior_ids or (None, None)))
    if prior_w is not None and k1:
        lam[0] = prior_w
    if prior_v is not None:
        lam[1:] = prior_v
    base, A, B = frozen_sums(model, frozen)
    nc = D_out - D
    out = dict(mu_w=np.zeros(nc), sigma_w=np.zeros(nc), mu_v=np.zeros((k, nc)), sigma_v=np.zeros((k, nc)),
               resid=np.zeros(n), prior_used=lam, col_passes=np.zeros(nc, dtype=np.int64))
    st = dict(new_attributes=nc, with_rows=0, longest_column=0, passes_max=0, not_converged=0, rows=n, nonfinite_updates=0)
    for c in range(nc):
        idx = np.nonzero(new_id == D + c)[0]          # ascending: the caller's order
        r = sweep_column(new_x[idx], target[idx], base[idx], A[idx], B[idx], lam, model["alpha"], k1, passes, tol)
        if solve and len(idx):
            r["w"], r["v"] = solve_column(new_x[idx], target[idx], base[idx], A[idx], B[idx], lam, model["alpha"], k1)
        out["mu_w"][c], out["sigma_w"][c] = (r["w"], r["s_w"]) if k1 else (0.0, 0.0)
        out["mu_v"][:, c], out["sigma_v"][:, c] = r["v"], r["s_v"]
        out["resid"][idx] = r["e"]
        out["col_passes"][c] = r["passes"]
        st["with_rows"] += len(idx) > 0
        st["longest_column"] = max(st["longest_column"], len(idx))
        st["passes_max"] = max(st["passes_max"], r["passes"])
        st["nonfinite_updates"] += r["nonfinite"]
        st["not_converged"] += int(tol > 0.0 and len(idx) > 0 and not r["converged"])
    out["stats"] = st
    return out


def extended(model, folded):
    """The parameters of the extended model: the input's, then the new ids'."""
    info = dict(model["info"])
    k, D = info["num_factor"], info["num_attribute"]
    nc = len(folded["mu_w"])
    info["num_attribute"] = D + nc
    p = dict(model, info=info)
    p["mu_w"] = np.concatenate([model["mu_w"], folded["mu_w"]])
    p["sigma_w"] = np.concatenate([model["sigma_w"], folded["sigma_w"]])
    p["mu_v"] = np.concatenate([model["mu_v"].reshape(k, D), folded["mu_v"]], axis=1).ravel()
    p["sigma_v"] = np.concatenate([model["sigma_v"].reshape(k, D), folded["sigma_v"]], axis=1).ravel()
    return p


def score(model, rows):
    """The unclipped mean of rows whose ids the model all has."""
    row_ptr, feat, val = rows
    frozen = []
    for r in range(len(row_ptr) - 1):
        b, e = int(row_ptr[r]), int(row_ptr[r + 1])
        ids, xs = np.asarray(feat[b:e], dtype=np.int64), np.asarray(val[b:e], dtype=np.float32)
        order = np.argsort(ids, kind="stable")
        frozen.append((ids[order], xs[order]))
    return frozen_sums(model, frozen)[0]

"""The chains that hold VBFM_RNG_DEVICE to the CPU oracle (tests/test_device_rng_cpu.py decides
which are eligible, tests/test_device_rng_gpu.py runs them on the device): the cases, their data,
and the oracle's side of a chain -- oracle_ctypes.ALS started from given parameters, its
per-attribute normals and task c's latent targets served by tests/keyed_rng.py."""
import os

import numpy as np

import class_ref as cr
import keyed_rng as kr
import oracle_ctypes as oc
import synth

TESTS = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(TESTS, "golden")

PERTURB = 4e-16       # relative change of a normal that the device's log / cos / sqrt cannot exceed
ELIGIBLE = 1e-11      # two oracle chains whose normals differ by PERTURB agree to this: 1/100 of 1e-9
MIN_DIST = 1e-9       # every accept / reject comparison of task c's draws is farther than this from its boundary

SYN = dict(rows=5000, fields=3, ids=50, test_rows=500, seed=31, test_seed=32, threshold=3.0)


class Case:
    def __init__(self, name, data, dim, seed, iters, init_stdev=0.1, task="r", method="mcmc", rng="device",
                 regular=(), meta=None, layouts=("auto",), threshold=None):
        self.name, self.data, self.dim, self.seed, self.iters = name, data, tuple(dim), seed, iters
        self.init_stdev, self.task, self.method, self.rng = init_stdev, task, method, rng
        self.regular, self.meta, self.layouts, self.threshold = tuple(regular), meta, tuple(layouts), threshold

    def __repr__(self):
        return self.name


# 4a: regression. tiny/mcmc's k = 3 over 6 iterations includes the sweeps whose stream ids were the
# initialisation's (21, 22) before those moved to bit 62. Seeds, dims and iteration counts are the
# fixtures' (tests/golden/*/trace.json), so REL is tests/test_mcmc_gpu.py's bound for the same runs.
REGRESSION = [
    Case("tiny/mcmc", "tiny", (1, 1, 3), 5, 6),
    Case("tiny_dup/mcmc", "tiny_dup", (1, 1, 3), 5, 6),
    Case("tiny/mcmc_meta", "tiny", (1, 1, 2), 11, 5, init_stdev=0.2, meta="groups.meta"),
    Case("synth_mcmc", "synth", (1, 1, 4), 7, 5, layouts=("level", "column")),
    Case("tiny/k0", "tiny", (1, 1, 0), 5, 6),
    Case("tiny/k1", "tiny", (1, 1, 1), 5, 6),
]

# 4d: task c. The 5,000-row set on both layouts; the fixtures' cls_tiny (entry store) and
# cls_tiny_dup (column layout, a repeated id); als on the reference stream.
CLASSIFICATION = [
    Case("syn5000/mcmc", "syn", (1, 1, 2), 20261021, 3, task="c", layouts=("auto", "column")),
    Case("cls_tiny/mcmc", "tiny", (1, 1, 4), 1792455606, 6, task="c", threshold=4.0),
    Case("cls_tiny_dup/mcmc", "tiny_dup", (1, 1, 4), 1792455609, 6, task="c", threshold=4.0),
    Case("cls_tiny/als_reg", "tiny", (1, 1, 4), 1792455606, 6, task="c", method="als", rng="reference",
         regular=(0.5, 1.0, 2.0), threshold=4.0),
    Case("syn5000/als", "syn", (1, 1, 2), 20261021, 3, task="c", method="als", rng="reference",
         regular=(0.5, 1.0, 2.0), layouts=("auto", "column")),
]

# Cases test_device_rng_cpu.py::test_chain_is_eligible found unstable (a 4e-16 change of the normals
# moves the chain by more than 1e-11 within the iterations run), as tiny_dup/als is in
# tests/test_mcmc_gpu.py: held on the oracle only. None so far.
DROPPED = ()


def by_name(name):
    return next(c for c in REGRESSION + CLASSIFICATION if c.name == name)


def syn_csr():
    """The 5,000-row field data with targets binarised at 3.0 on the host, and its test rows."""
    out = []
    for n, seed in ((SYN["rows"], SYN["seed"]), (SYN["test_rows"], SYN["test_seed"])):
        rp, f, v, y = synth.generate(n, SYN["fields"], SYN["ids"], seed, 0)
        out.append((n, rp, f, v, np.where(y >= SYN["threshold"], 1.0, -1.0).astype(np.float32)))
    return out


def sources(case, tmpdir, synth_files):
    """(train, test) as a path or a CSR tuple (n, row_ptr, feat, val, y)."""
    if case.data == "syn":
        return tuple(syn_csr())
    if case.data == "synth":
        return synth_files["train"], synth_files["test"]
    if case.threshold is not None:
        f = cr.case_files(tmpdir, case.data, case.threshold)
        return f["train"], f["test"]
    d = os.path.join(GOLDEN, case.data)
    return os.path.join(d, "train.libfm"), os.path.join(d, "test.libfm")


def oracle_data(src):
    return tuple(oc.Data(s) if isinstance(s, str) else oc.Data(csr=s) for s in src)


def groups_of(case, D):
    if case.meta is None:
        return None
    g = np.loadtxt(os.path.join(GOLDEN, case.data, case.meta), dtype=np.uint32)
    assert len(g) == D
    return g


def start_params(case, D, G):
    """What vbfm_mcmc_init leaves in device mode, by the restatement: fm.w / fm.v from the
    initialisation streams, the hyper-priors of fm_learn_mcmc::init."""
    k = case.dim[2]
    w, v = kr.init_params(case.seed, case.init_stdev, k, D)
    return {"w": w, "v": v, "w_mu": np.zeros(G), "w_lambda": np.zeros(G), "v_mu": np.zeros(G * k),
            "v_lambda": np.zeros(G * k), "w0": 0.0, "alpha": 1.0}


def perturbed(z, eps):
    return z + eps * np.maximum(1.0, np.abs(z)) if eps else z


def oracle_chain(case, train, test, start=None, eps=0.0, iters=None):
    """The oracle's chain: a list with one snapshot per iteration (parameters, hyper-priors, alpha,
    w0, e and the iteration's figures), and the learner. rng "device": started from `start`, the
    normals of the sweeps from the restatement (moved by eps, test_device_rng_cpu.py), task c's
    latent targets from the restatement on the oracle's own yhat; snapshot["dist"] is then the
    smallest decision distance over the rows. rng "reference": the or_srand stream throughout."""
    k0, k1, k = case.dim
    D = oc.num_all_attribute(train, test)
    groups = groups_of(case, D)
    reg = list(case.regular) or [0.0, 0.0, 0.0]
    o = oc.ALS(k0, k1, k, D, groups, method=case.method, reg0=reg[0], task=case.task)
    dist = {}
    if case.rng == "device":
        o.seed(case.seed)
        o.set_params(start if start is not None else start_params(case, D, o.s.G))
        o.set_normal_source(lambda it, f, n: perturbed(kr.sweep_normals(case.seed, it, f, k, n), eps))
        if case.task == "c":
            def latent(it, yhat, pos):
                s, _, flag, d = kr.class_sample_target(yhat, pos, case.seed, kr.CLASS_STREAM | it, np.arange(len(yhat)))
                assert not flag.any()
                dist[it] = float(d.min())
                return s
            o.set_latent_source(latent)
    else:
        o.init_params(case.seed, case.init_stdev)
        o.set_lambda(np.full(o.s.G, reg[1]), np.full(o.s.G * k, reg[2]))
    o.attach(train, test)
    snaps = []
    for it in range(case.iters if iters is None else iters):
        rmse_all, rmse_this, train_rmse = o.iterate()
        s = o.params()
        s["e"] = o.rows()["e"]
        if case.task == "c":
            s.update(o.class_info())
            s["dist"] = dist.get(it, np.inf)
        else:
            s.update(rmse_all=rmse_all, rmse_this=rmse_this, train_rmse=train_rmse)
        snaps.append(s)
    return snaps, o


ARRAYS = ("w", "v", "w_mu", "w_lambda", "v_mu", "v_lambda", "e")
SCALARS = {"r": ("alpha", "w0", "rmse_all", "rmse_this", "train_rmse"), "c": ("alpha", "w0", "ll_this", "ll_all")}
COUNTS = ("n_train_correct", "n_test_correct_this", "n_test_correct_all")


def rel_err(a, b):
    """max |a - b| / max |b|: tests/test_mcmc_gpu.py's measure. Both sides must be finite and of
    one shape: a NaN would otherwise pass every `<=` fold silently."""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.isfinite(a).all() and np.isfinite(b).all(), "non-finite value"
    if b.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b))) / max(1e-300, float(np.max(np.abs(b))))


def compare(task, got, want, worst, bound):
    """Relative errors of one iteration's snapshot `got` against the oracle's `want`: each must be
    finite and within `bound` (asserted here, per quantity), then it is folded into worst[name] for
    the report; the counts of task c must be equal."""
    for key in ARRAYS + SCALARS[task]:
        try:
            err = rel_err(got[key], want[key])
        except AssertionError as exc:
            raise AssertionError("%s: %s" % (key, exc))
        assert np.isfinite(err) and err <= bound, (key, err, bound)
        worst[key] = max(worst.get(key, 0.0), err)
    if task == "c":
        for key in COUNTS:
            assert got[key] == want[key], (key, got[key], want[key])
    return worst

"""Every lane-group width of the online learner against the CPU oracle.

A level kernel of the online learner serves one column with G lanes; G comes from the level's
floor(mean column length) / num_batch (ov_level for the column kernels k_ov_{w,v}_level, ov_lord_g
for k_ov_lord on the per-batch level-ordered store; csrc/vbfm_online.hip, restated as
synth.OV_G_TABLE / OV_LORD_G_TABLE). G decides the butterfly depth, the columns per workgroup
(256 / G, so the dead lane groups of a level's last workgroup), which entries sit in the two register
slots and which go through the loop, and the size of a workgroup's run in the padded layout.
tests/test_online_gpu.py compares with a reference only at G = 4.

Here every G in 4, 8, 16, 32, 64 runs on a data set of its own (tests/online_cases.py): three one-hot
fields, each a level with more than 256 / G columns of 1, G - 1, G, G + 1, 2 G, 2 G + 1 and 3 G + 1
entries. With one batch those lengths are exact; with two (every length doubled, one column of
length 1 kept and so empty in one batch) the natural parameters' carry-over, the step sizes, both
free energies and a column absent from a batch take part. The wide set (columns up to 520) runs
the 256-lane column kernel, and on the store k_ov_lord<64> with runs beyond OV_CAP, which also sends
every batch from the padded to the packed layout. Each run first asserts, from the learner's own
levels() and CSC, that the width is the intended one, and from every epoch's statistics that the
form (padded / packed / column) is; tests/test_online_shapes_cpu.py checks the same without a GPU.

Every epoch's test RMSE and free energies and the final parameters, natural parameters, step sizes,
scalars and predictions are held to the oracle at REL = 1e-9, the bound of tests/test_online_gpu.py
(tree against sequential column sums); the three store forms are bit-identical to each other. A
record lost from a 3 G + 1 column moves the oracle's own parameters by more than a thousand times
that bound (tests/test_online_shapes_cpu.py). Every test prints its largest error per quantity.

What these cases decide, tried on scratch builds: group_sum2's butterfly one step short at G = 16
alone fails the 24 g16 cases by 5e-2 .. 4 relative; the second register entry taken for
lane + G <= n at G = 64 alone fails the eight g64 column cases by 4e-4 .. 4e-2; a corrected record at
run position OV_CAP - 1 written past its staged copy fails the six wide store cases by 2e-3 .. 0.4.
The tests that existed before pass all three.
"""
import numpy as np
import pytest

import online_cases as ocs
import vbfm
from test_online_gpu import REL, check_final, rel_err

pytestmark = pytest.mark.gpu

# the learner's forms: the environment that selects each, and what every epoch's statistics must say
FORMS = {
    "padded": {},                          # padded store, tagged arguments on the v levels
    "plain-args": {"VBFM_OV_FAST": "0"},   # padded store, k_ov_lord's plain arguments everywhere
    "packed": {"VBFM_OV_PAD": "0"},        # the store with packed runs at every level
    "column": {"VBFM_LAYOUT": "column"},   # k_ov_{w,v}_level: no store
}
STORE_FORMS = ("padded", "plain-args", "packed")
WIDTH_SETS = ocs.SETS[:-1]
widths = pytest.mark.parametrize("name", WIDTH_SETS)
batches = pytest.mark.parametrize("nb", [1, 2], ids=["b1", "b2"])

_runs = {}


class _Run:
    """What a run left: every epoch's statistics and the final state, read as check_final reads a
    learner's."""

    def __init__(self, stats, params, state, pred):
        self.stats, self.params, self.state, self.pred = stats, params, state, pred

    def get_params(self):
        return self.params

    def online_state(self):
        return self.state

    def predict(self):
        return self.pred


def _run(name, nb, k, xmode, form, grouped, monkeypatch):
    """ITERS epochs of the learner in `form`; computed once per process (the bit-identity tests
    compare the runs the oracle tests made)."""
    key = (name, nb, k, xmode, form, grouped)
    if key in _runs:
        return _runs[key]
    for var in ocs.ONLINE_ENV:
        monkeypatch.delenv(var, raising=False)
    for var, value in FORMS[form].items():
        monkeypatch.setenv(var, value)
    tr, te, nf, nft, D = ocs.data(name, nb, xmode)
    train, test = vbfm.DataSubset.from_csr(*tr, nf), vbfm.DataSubset.from_csr(*te, nft)
    g = vbfm.FMLearnVBOnline(1, 1, k, D, attr_group=ocs.field_groups(name, nb) if grouped else None,
                             min_target=train.min_target, max_target=train.max_target)
    g.set_data(train, test)
    g.init(ocs.SEED, ocs.INIT_STDEV, nb)
    lv, L = g.levels()
    cp, ent, _ = g.get_csc(0)
    ocs.check_conditions(name, nb, lv, L, cp, ent["id"])
    assert bool((ent["value"] == 1).all()) == (xmode == 0)
    stats = []
    for it in range(ocs.ITERS):
        st = g.epoch()
        assert st.num_batch == nb
        if form == "column":
            assert st.n_lord_batches == 0, (it, st.n_lord_batches)
        else:
            assert st.n_lord_batches == nb, (it, st.n_lord_batches)
            padded = form != "packed" and name != "wide"      # the wide set's runs exceed OV_CAP
            assert st.n_pad_batches == (nb if padded else 0), (it, st.n_pad_batches)
        stats.append((st.rmse, st.mae, st.free_energy_first, st.free_energy_last, st.alpha))
    p, s = g.get_params(), g.online_state()
    res = _Run(stats, {key: np.array(v) for key, v in p.items()}, {key: np.array(v) for key, v in s.items()},
               np.array(g.predict()))
    g.close()
    _runs[key] = res
    return res


def _vs_oracle(name, nb, k, xmode, form, grouped, monkeypatch):
    out, op, _ = ocs.oracle_run(name, nb, k, xmode, grouped)
    res = _run(name, nb, k, xmode, form, grouped, monkeypatch)
    errs = {"rmse": 0.0, "free energy": 0.0}
    for st, (rmse, _, fe_first, fe_last) in zip(res.stats, out):
        errs["rmse"] = max(errs["rmse"], rel_err(st[0], rmse))
        fe, ref = ([st[2]], [fe_first]) if nb == 1 else ([st[2], st[3]], [fe_first, fe_last])
        errs["free energy"] = max(errs["free energy"], rel_err(fe, ref))
    p, s = res.params, res.state
    for key in ("mu_w", "sigma_w", "mu_v", "sigma_v", "hyp_sigma_w", "hyp_sigma_v"):
        errs[key] = rel_err(p[key], op[key])
    for key in ("nat_mu_w", "nat_sigma_w", "nat_mu_v", "nat_sigma_v", "scalars"):
        errs[key] = rel_err(s[key], op[key])
    errs["steps"] = rel_err(np.concatenate([s["new_wj"], s["new_vj"]]), op["steps"])
    errs["pred"] = rel_err(res.pred, op["pred"])
    print("online %s b%d k=%d x%d %s%s:" % (name, nb, k, xmode, form, " groups" if grouped else ""),
          " ".join("%s %.2e" % kv for kv in errs.items()))
    for key in ("rmse", "free energy"):
        assert errs[key] <= REL, (key, errs[key])
    check_final(res, {}, op)


def _bit_identical(name, nb, k, xmode, forms, grouped, monkeypatch):
    res = [_run(name, nb, k, xmode, form, grouped, monkeypatch) for form in forms]
    for form, r in zip(forms[1:], res[1:]):
        assert r.stats == res[0].stats, form
        for part in ("params", "state"):
            for key, v in getattr(res[0], part).items():
                np.testing.assert_array_equal(getattr(r, part)[key], v, err_msg="%s %s" % (form, key))
        np.testing.assert_array_equal(r.pred, res[0].pred, err_msg=form)


@pytest.mark.parametrize("form", list(FORMS))
@batches
@widths
def test_width_vs_oracle(name, nb, form, monkeypatch):
    """k = 3 (w with a next factor, both q-cache slots with one, the last factor without), stored x."""
    _vs_oracle(name, nb, 3, 1, form, False, monkeypatch)


@batches
@widths
def test_store_forms_bit_identical(name, nb, monkeypatch):
    """The padded layout, the plain arguments and the packed layout move the same records through
    the same lanes: epochs, parameters and online state equal bit for bit, at every width."""
    _bit_identical(name, nb, 3, 1, STORE_FORMS, False, monkeypatch)


@pytest.mark.parametrize("form", ["padded", "column"])
@batches
@widths
def test_unit_x_vs_oracle(name, nb, form, monkeypatch):
    """Every x is 1: k_ov_lord loads no x (a.x_one)."""
    _vs_oracle(name, nb, 3, 0, form, False, monkeypatch)


@pytest.mark.parametrize("k", [1, 2])
@widths
def test_few_factors_vs_oracle(name, k, monkeypatch):
    """Slot 0 (k = 1) and slot 1 (k = 2) without a next factor."""
    _vs_oracle(name, 2, k, 1, "padded", False, monkeypatch)


@pytest.mark.parametrize("form", ["padded", "column"])
@batches
@widths
def test_no_factors_vs_oracle(name, nb, form, monkeypatch):
    """k = 0: the w kernels alone, without a next factor."""
    _vs_oracle(name, nb, 0, 1, form, False, monkeypatch)


@pytest.mark.parametrize("form", ["padded", "plain-args", "column"])
@batches
@pytest.mark.parametrize("name", ["g16", "g64"])
def test_attribute_groups_vs_oracle(name, nb, form, monkeypatch):
    """One attribute group per field: the per-column prior follows attr_group (!a.hyp_uniform)."""
    _vs_oracle(name, nb, 3, 1, form, True, monkeypatch)


@pytest.mark.parametrize("xmode", [1, 0], ids=["x1", "x0"])
@pytest.mark.parametrize("form", ["column", "padded", "packed"])
def test_wide_vs_oracle(form, xmode, monkeypatch):
    """Columns up to 520 entries in one batch: the 256-lane column kernel (form column), and on the
    store k_ov_lord<64> with runs beyond OV_CAP, read and written past the staged records. With
    nothing set (form padded) k_ov_pad_check (csrc/vbfm_online_batch.hip) sends the batch to the packed
    layout."""
    _vs_oracle("wide", 1, 3, xmode, form, False, monkeypatch)


@pytest.mark.parametrize("xmode", [1, 0], ids=["x1", "x0"])
def test_wide_store_forms_bit_identical(xmode, monkeypatch):
    """The batch that fell back from the padded layout is the packed run bit for bit."""
    _bit_identical("wide", 1, 3, xmode, ("padded", "packed"), False, monkeypatch)

"""bin/libFM -load_model M -fold_in S -save_model M2 -test T -out P on the GPU: the extended model's file
and the scores are those of the Python path (Model.fold_in, Model.save, Model.score) on the same
files. Tiny data: the held-out users of tests/fold_in_cases.py."""
import os
import subprocess

import numpy as np
import pytest

import fold_in_cases as fc
import synth
import vbfm
from conftest import ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "scalable-variational-bayesian-factorization-machine_amd", "bin", "libFM")


def test_cli_fold_in_is_the_python_path(tmp_path):
    D, block, train, (s_rows, s_y), (t_rows, t_y) = fc.heldout_set()
    info, p = fc.heldout_model(D, train, iters=5)
    model, support, test = (str(tmp_path / n) for n in ("m", "support.libfm", "test.libfm"))
    vbfm.Model.write_params(model, info, p)
    synth.write_libfm(support, *s_rows, s_y)
    synth.write_libfm(test, *t_rows, t_y)
    r = subprocess.run([CLI, "-load_model", model, "-fold_in", support, "-fold_passes", "7", "-fold_tol", "1e-9",
                        "-fold_prior_ids", "%d,%d" % block, "-save_model", "m2", "-test", test, "-out", "p"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = vbfm.Model.load(model)
    ext, st = m.fold_in(vbfm.DataSubset.load(support), passes=7, tol=1e-9, prior_ids=block)
    line = "folded in %d new attributes from %d rows: at most %d passes, %d columns not converged" % (
        st["new_attributes"], st["rows"], st["passes_max"], st["not_converged"])
    assert line in r.stdout, r.stdout[-2000:]
    ext.save(str(tmp_path / "m2_py"))
    assert open(tmp_path / "m2", "rb").read() == open(tmp_path / "m2_py", "rb").read()
    want = ext.score(vbfm.DataSubset.load(test))
    got = open(tmp_path / "p").read().split()
    assert got == ["%g" % v for v in want]
    # without a test set: the extended model alone, the same file
    r = subprocess.run([CLI, "-load_model", model, "-fold_in", support, "-fold_passes", "7", "-fold_tol", "1e-9",
                        "-fold_prior_ids", "%d,%d" % block, "-save_model", "m3"], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert open(tmp_path / "m3", "rb").read() == open(tmp_path / "m2_py", "rb").read()
    # the loaded model alone refuses the new ids
    r = subprocess.run([CLI, "-load_model", model, "-test", test, "-out", "q"], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=300)
    assert "ERROR: row 0 holds feature id" in r.stderr and not os.path.exists(tmp_path / "q")

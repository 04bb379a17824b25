"""bin/libFM's host code pinned on the CPU: host/libfm_main.cpp linked with the stand-ins
tests/cli_stub.cpp + tests/cli_stub_model.cpp (every learner, the model and chain entry points) under
ASan + UBSan with leak detection, run over the matrix of tests/cli_stub_cases.py and compared with the
records under tests/golden/cli_stub/ (tests/golden/make_cli_stub_golden.py): stdout, stderr, the exit
status, every file a run leaves and every rank's calls into the library, in order. The stand-ins put a
distinct value into every field of every stats struct, so a value printed under another's key shows.
"""
import json
import os
import shutil

import pytest

import cli_stub_cases as cc
from test_host_sanitizers import SAN

pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="needs g++")

SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """a stand-alone executable with the sanitizer runtimes linked statically; nothing is preloaded"""
    path = str(tmp_path_factory.mktemp("cli_stub") / "libfm_stub_san")
    cc.build(cc.LAUNCHER, path, [*SAN, "-static-libasan", "-static-libubsan"])
    return path


@pytest.fixture(scope="module")
def records(exe):
    done = {}

    def get(name):
        if name not in done:
            done[name] = cc.run_case(exe, name, SAN_ENV)
        return done[name]
    return get


@pytest.mark.parametrize("name", cc.RECORDED)
def test_launcher_matches_its_record(records, name):
    with open(cc.fixture_path(name)) as fh:
        want = json.load(fh)
    got = records(name)
    assert len(got) == len(want)
    for n, (g, w) in enumerate(zip(got, want)):
        for s in g["stderr"] + g["stdout"]:
            assert "AddressSanitizer" not in s and "LeakSanitizer" not in s and "runtime error" not in s, \
                "%s step %d %s:\n%s" % (name, n, g["flags"], "".join(g["stderr"])[-6000:])
        for key in ("flags", "env", "exit", "stdout", "stderr", "traces"):
            assert g[key] == w[key], "%s step %d %s: %s differs" % (name, n, g["flags"], key)
        assert sorted(g["files"]) == sorted(w["files"]), "%s step %d %s: files left" % (name, n, g["flags"])
        for f in w["files"]:
            assert g["files"][f] == w["files"][f], "%s step %d %s: file %s differs" % (name, n, g["flags"], f)


@pytest.mark.parametrize("name", cc.ERROR_CASES)
def test_failure_ends_with_its_error_line_and_status_0(records, name):
    for g in records(name):
        assert g["exit"] == 0, "".join(g["stderr"])[-6000:]
        assert any(s.startswith("ERROR: ") for s in g["stderr"]), g["stderr"]
        assert not any("Sanitizer" in s or "runtime error" in s for s in g["stderr"]), g["stderr"]
        if name in cc.UNORDERED:
            assert "of 2 failed (exit status 1); the other ranks were stopped" in g["stderr"][-1], g["stderr"]


def test_stand_ins_fill_every_field_distinctly():
    """what makes the records a check of the wiring: within one -parity_log line no two keys share a
    value (bar the documented derived ones), none is 0 or null, and values move with the iteration"""
    for name, fname in (("vb_host", "parity.jsonl"), ("mcmc", "parity.jsonl"), ("mcmc_c", "parity.jsonl"),
                        ("online_b3", "parity.jsonl")):
        with open(cc.fixture_path(name)) as fh:
            lines = [json.loads(s) for s in json.load(fh)[0]["files"][fname]]
        its = [r for r in lines if r["method"] != "setup"]
        assert lines[0]["method"] == "setup" and len(its) == 3
        for r in lines:
            vals = {k: v for k, v in r.items() if k not in ("method", "learner", "iter", "load_s", "sweep_nnz_k_per_s",
                                                             "hbm_frac_per_gpu")}
            if r["method"] == "vb" and r["iter"] == 2:   # the iteration whose free energy is not valid
                assert vals.pop("free_energy") is None
            assert all(v is not None and v != 0 for v in vals.values()), r
            assert len(set(vals.values())) == len(vals), r
            assert r["method"] == "setup" or r["sweep_nnz_k_per_s"] > 0
        moving = [k for k in its[0] if k not in ("method", "train", "test_rmse", "free_energy") and its[0][k] is not None]
        assert all(its[0][k] != its[1][k] for k in moving), (its[0], its[1])

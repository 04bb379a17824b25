"""bin/libFM's -candidates / -topn / -exclude flags without a GPU: host/libfm_main.cpp linked with
tests/cli_stub.cpp (the compile line of test_model_cpu.test_cli_without_the_scorer_says_so), which
has none of the model, scoring or recommendation entry points. The flag refusals are decided before
any of them is needed; a well-formed -candidates run ends in the "no scorer" message."""
import os
import subprocess

import pytest

from conftest import ROOT, TESTS

PKG = os.path.join(ROOT, "scalable-variational-bayesian-factorization-machine_amd")
TINY = os.path.join(TESTS, "golden", "tiny")
TRAIN, TEST = os.path.join(TINY, "train.libfm"), os.path.join(TINY, "test.libfm")


@pytest.fixture(scope="module")
def stub_cli(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stub") / "libfm_stub")
    subprocess.run(["g++", "-std=c++17", "-O0", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(PKG, "host", "libfm_main.cpp"), os.path.join(PKG, "csrc", "vbfm_host.cpp"),
                    os.path.join(TESTS, "cli_stub.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    return exe


def run(exe, args, cwd):
    return subprocess.run([exe] + args, cwd=str(cwd), capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("extra,message", [
    (["-topn", "3"], "-topn needs -candidates"),
    (["-exclude", "x"], "-exclude needs -candidates"),
    (["-candidates", TRAIN], "-candidates needs -topn"),
    (["-candidates", TRAIN, "-topn", "3", "-out_var", "v"], "-out_var does not apply to -candidates"),
])
def test_flag_refusals_inside_load_model(stub_cli, tmp_path, extra, message):
    r = run(stub_cli, ["-load_model", "m", "-test", TEST, "-out", "p"] + extra, tmp_path)
    assert "ERROR: " + message in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(tmp_path / "p")


@pytest.mark.parametrize("extra", [["-candidates", TRAIN, "-topn", "3"], ["-topn", "3"], ["-exclude", "x"],
                                   ["-candidates", TRAIN]])
def test_the_flags_are_refused_outside_load_model(stub_cli, tmp_path, extra):
    r = run(stub_cli, ["-task", "r", "-train", TRAIN, "-test", TEST, "-method", "vb", "-dim", "1,1,2", "-iter", "1",
                       "-seed", "3"] + extra, tmp_path)
    assert "ERROR: -candidates, -topn and -exclude belong to -load_model" in r.stderr, r.stderr[-2000:]


def test_candidates_without_the_scorer_says_so(stub_cli, tmp_path):
    r = run(stub_cli, ["-load_model", "m", "-test", TEST, "-candidates", TRAIN, "-topn", "3", "-out", "p"], tmp_path)
    assert "ERROR: this build has no scorer" in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(tmp_path / "p")


def test_help_lists_the_flags(stub_cli, tmp_path):
    r = run(stub_cli, ["-help"], tmp_path)
    for flag in ("-candidates", "-topn", "-exclude"):
        assert flag in r.stdout + r.stderr

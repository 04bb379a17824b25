#!/usr/bin/env python3
"""Generate the launcher's CPU fixtures tests/golden/cli_stub/<case>.json: what bin/libFM's host
code (host/libfm_main.cpp) prints, writes and calls, per rank and in order, when it is linked with
the stand-ins tests/cli_stub.cpp + tests/cli_stub_model.cpp in place of the GPU library and run over
the matrix of tests/cli_stub_cases.py (every learner, resume, several ranks, -task c, -chain, the
failure paths). The build is a plain one (no sanitizer); tests/test_cli_stub_cpu.py builds the same
sources under ASan + UBSan and asserts equality with these records.

The fixtures are a record of the launcher BEFORE a change to it: generate them from the source file
of the commit the change starts from, e.g.

    git show HEAD:scalable-variational-bayesian-factorization-machine_amd/host/libfm_main.cpp > /tmp/parent.cpp
    python tests/golden/make_cli_stub_golden.py /tmp/parent.cpp

and a refactored launcher must reproduce them with an empty `git diff`. Default: the tree's.

Usage: python tests/golden/make_cli_stub_golden.py [LAUNCHER.cpp] [--only case,case]
"""
import argparse
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cli_stub_cases as cc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("launcher", nargs="?", default=cc.LAUNCHER, help="the launcher's source file")
    ap.add_argument("--only", default="", help="comma list of case names")
    a = ap.parse_args()
    only = set(filter(None, a.only.split(",")))
    tmp = tempfile.mkdtemp(prefix="cli_stub_build_")
    try:
        exe = os.path.join(tmp, "libfm_stub")
        cc.build(os.path.abspath(a.launcher), exe, ["-O1", "-g"])
        os.makedirs(cc.FIXTURES, exist_ok=True)
        for name in cc.RECORDED:
            if only and name not in only:
                continue
            with open(cc.fixture_path(name), "w") as fh:
                fh.write(cc.dump(cc.run_case(exe, name)))
            print(name, "ok")
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()

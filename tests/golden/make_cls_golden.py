#!/usr/bin/env python3
"""Generate the binary-classification fixtures tests/golden/cls_<case>/{trace.json, pred.npy} from the
COMPILED REFERENCE CLI (oracle/_ref/libFM, built by `make -C oracle ref`; the reference itself
never travels), run unmodified with -task c.

Every case thresholds the targets of an existing fixture's inputs (target >= 4 -> 1, else -1),
which a test derives again with the same helper (tests/class_ref.py write_thresholded), so no input
files are stored. A trace holds

  meta     the command line's values, the data set, the threshold, the row counts
  iters    per iteration: train / test accuracy of the "#Iter=" line, and the -rlog columns the
           reference initialises (accuracy, acc_mcmc_this, acc_mcmc_all, ll_mcmc_this, alpha,
           wmu / wlambda / vmu / vlambda)
  pred.npy the -out file (probabilities), float64, beside the trace

all at the reference's 6 significant digits. A case is refused if the run printed a #nans / #inf
line.

The seed: the reference CLI ignores -seed and calls srand(time(NULL)) as its first statement
(libfm.cpp:123-124). The binary is started in the middle of a clock second (time() reads a coarse
clock that can lag a few milliseconds behind, so not near a boundary) and that epoch second is
recorded as the case's seed (meta.seed), which the drop-in's -seed / vbfm_mcmc_config then
replays; the run is discarded unless the process was up within the same half second.

The reference's MAP@5 reads a side file from a fixed path that does not exist here; its reader
breaks out at once and the field prints 0.

Usage: python tests/golden/make_cls_golden.py [--ref oracle/_ref/libFM]
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import class_ref as cr  # noqa: E402

CASES = {
    "cls_tiny/mcmc": dict(data="tiny", method="mcmc", dim="1,1,4", iters=6, regular=None),
    "cls_tiny/als_reg": dict(data="tiny", method="als", dim="1,1,4", iters=6, regular="0.5,1,2"),
    "cls_sa/mcmc": dict(data="sa_split", method="mcmc", dim="1,1,8", iters=5, regular=None),
    "cls_sa/als_reg": dict(data="sa_split", method="als", dim="1,1,8", iters=5, regular="0,1,5"),
    "cls_tiny_dup/mcmc": dict(data="tiny_dup", method="mcmc", dim="1,1,4", iters=6, regular=None),
}
THRESHOLD = 4.0


def inputs(data):
    d = os.path.join(HERE, data)
    ext = ".libfm.gz" if data == "sa_split" else ".libfm"
    return os.path.join(d, "train" + ext), os.path.join(d, "test" + ext)


def run_case(ref, c):
    tmp = tempfile.mkdtemp(prefix="cls_golden_")
    try:
        tr, te = inputs(c["data"])
        n_train = cr.write_thresholded(tr, os.path.join(tmp, "train.libfm"), THRESHOLD)
        n_test = cr.write_thresholded(te, os.path.join(tmp, "test.libfm"), THRESHOLD)
        cmd = [ref, "-task", "c", "-train", "train.libfm", "-test", "test.libfm", "-method", c["method"], "-dim", c["dim"],
               "-iter", str(c["iters"]), "-out", "pred.txt", "-rlog", "rlog.tsv"]
        if c["regular"]:
            cmd += ["-regular", c["regular"]]
        for _ in range(20):
            while not 0.3 < time.time() % 1.0 < 0.4:     # mid-second: srand(time(NULL)) comes at once
                time.sleep(0.002)
            seed = int(time.time())
            proc = subprocess.Popen(cmd, cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            started = time.time()
            out, err = proc.communicate()
            if proc.returncode != 0:
                raise SystemExit("the reference failed:\n" + out[-2000:] + err[-2000:])
            if int(started) == seed and started - seed < 0.8:
                break
        else:
            raise SystemExit("could not start the reference within one clock second")
        res = subprocess.CompletedProcess(cmd, 0, out, err)
        if re.search(r"#nans|#inf", res.stdout):
            raise SystemExit("the reference reported NaN / inf draws: not a fixture\n" + res.stdout[-2000:])
        iters = []
        for m in re.finditer(r"#Iter=\s*(\d+)\tTrain=(\S+)\tTest=(\S+)", res.stdout):
            iters.append({"iter": int(m.group(1)), "train_acc": float(m.group(2)), "test_acc": float(m.group(3))})
        assert len(iters) == c["iters"], res.stdout[-2000:]
        with open(os.path.join(tmp, "rlog.tsv")) as fh:
            head = fh.readline().rstrip("\n").split("\t")
            rows = [ln.rstrip("\n").split("\t") for ln in fh if ln.strip()]
        assert len(rows) == c["iters"], (len(rows), c["iters"])
        keep = [h for h in head if h in ("accuracy", "acc_mcmc_this", "acc_mcmc_all", "ll_mcmc_this", "alpha")
                or re.match(r"(wmu|wlambda|vmu|vlambda)\[", h)]
        for it, row in zip(iters, rows):
            vals = dict(zip(head, row))
            it["rlog"] = {h: float(vals[h]) for h in keep}
        with open(os.path.join(tmp, "pred.txt")) as fh:
            pred = [float(x) for x in fh.read().split()]
        assert len(pred) == n_test
        k0, k1, k = (int(x) for x in c["dim"].split(","))
        meta = {"data": c["data"], "threshold": THRESHOLD, "method": c["method"], "dim": [k0, k1, k],
                "iter": c["iters"], "seed": seed, "init_stdev": 0.1,
                "regular": [float(x) for x in c["regular"].split(",")] if c["regular"] else [],
                "n_train": n_train, "n_test": n_test}
        return {"meta": meta, "iters": iters, "pred": pred}
    finally:
        shutil.rmtree(tmp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.path.join(ROOT, "oracle", "_ref", "libFM"))
    ap.add_argument("--only", default="", help="comma list of case names")
    a = ap.parse_args()
    only = set(filter(None, a.only.split(",")))
    for name, c in CASES.items():
        if only and name not in only:
            continue
        t = run_case(os.path.abspath(a.ref), c)
        d = os.path.join(HERE, name)
        os.makedirs(d, exist_ok=True)
        np.save(os.path.join(d, "pred.npy"), np.asarray(t.pop("pred"), dtype=np.float64))
        with open(os.path.join(d, "trace.json"), "w") as fh:   # one line per iteration
            fh.write('{"meta": %s,\n "iters": [\n  %s\n ]}\n' % (json.dumps(t["meta"]),
                                                                ",\n  ".join(json.dumps(i) for i in t["iters"])))
        print(name, "ok:", t["iters"][-1])


if __name__ == "__main__":
    main()

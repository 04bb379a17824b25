"""The launcher's CPU fixture (tests/golden/cli_stub/): host/libfm_main.cpp linked with the stand-ins
tests/cli_stub.cpp + tests/cli_stub_model.cpp instead of the GPU library, run over a matrix of
command lines. Shared by the generator (tests/golden/make_cli_stub_golden.py) and the test
(tests/test_cli_stub_cpu.py): the cases, how one is run and what is normalised.

A case is a list of steps run one after another in one fresh directory. Of every step the record
holds the flags, stdout, stderr, the exit status, every file in the directory afterwards (by name)
and each rank's call trace (VBFM_STUB_TRACE). Normalised, because a run cannot reproduce them: the
ctime line -method vb prints per iteration, the time_learn / time_learn2 / time_learn4 columns of
-rlog, and load_s of -parity_log's setup line. Every other byte is compared.
"""
import json
import os
import re
import shutil
import subprocess
import tempfile

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
PKG = os.path.join(ROOT, "scalable-variational-bayesian-factorization-machine_amd")
TINY = os.path.join(TESTS, "golden", "tiny")
FIXTURES = os.path.join(TESTS, "golden", "cli_stub")
LAUNCHER = os.path.join(PKG, "host", "libfm_main.cpp")

RLOG, NO_DIR = "log.tsv", "/nonexistent_dir/x.tsv"
ALL = ["-rlog", RLOG, "-out", "pred.txt", "-parity_log", "parity.jsonl", "-save_state", "st"]
META = ["-meta", os.path.join(TINY, "groups.meta")]
P3 = ["-devices", "3", "-transport", "host"]


def step(method, *flags, task="r", env=None):
    return {"flags": ["-task", task, "-method", method] + list(flags), "env": env or {}}


def _vb(pre, env=None):
    return [step("vb", "-init_stdev", "0.1", *pre, *ALL, *META, env=env),
            step("vb", *pre, "-resume", "st", "-rlog", RLOG, "-iter", "2", env=env),
            step("vb", *pre, "-vfile", "0", env=env)]


def _mcmc(method, pre):
    return [step(method, "-init_stdev", "0.1", *pre, *ALL, "-save_model", "m", *META),
            step(method, *pre, *ALL, "-save_model", "m", "-resume", "st"),
            step(method, *pre, *P3, *ALL, "-save_model", "m")]


def _online(batch):
    return [step("vb_online", "-batch", batch, "-init_stdev", "0.1", *ALL, "-save_model", "m", *META),
            step("vb_online", "-batch", batch, "-resume", "st", "-rlog", RLOG),
            step("vb_online", "-batch", batch, "-vfile", "0", env={"VBFM_INIT": "replay"})]


CASES = {
    "vb_host": _vb([], {"VBFM_INIT": "host"}),
    "vb_replay": _vb([], {"VBFM_INIT": "replay"}),
    "vb_p3": _vb(P3),
    "vb_p3_features": _vb(P3 + ["-shard", "features"]),
    "mcmc": _mcmc("mcmc", []),
    "als": _mcmc("als", ["-regular", "0,1,2"]),
    "mcmc_c": [step("mcmc", *ALL, "-save_model", "m", *META, task="c"),
               step("mcmc", "-devices", "2", "-transport", "host", *ALL, task="c")],
    "als_c": [step("als", *ALL, "-save_model", "m", task="c")],
    "mcmc_chain": [step("mcmc", "-chain", "1,2", "-save_model", "m", "-iter", "6")],
    "online_b3": _online("3"),
    "online_b1": _online("1"),
    # the failure paths: each ends with its ERROR: line and exit status 0, as the reference does
    "err_rlog": [step(m, "-rlog", NO_DIR) for m in ("vb", "mcmc", "als", "vb_online")],
    "err_resume": [step(m, "-resume", "missing") for m in ("vb", "mcmc", "vb_online")],
    "err_iterate": [step(m, *ALL, env={"VBFM_STUB_FAIL_ITER": "1"}) for m in ("vb", "mcmc", "vb_online")]
                   + [step("mcmc", "-chain", "0,1", "-save_model", "m", env={"VBFM_STUB_FAIL_ITER": "2"})],
    "err_rccl": [step("vb", "-devices", "2"), step("mcmc", "-devices", "2")],
    "err_online_ranks": [step("vb_online", *P3)],
}
ERROR_CASES = [c for c in CASES if c.startswith("err_")]
# Both ranks of err_rccl fail at once (rank 0: the stand-in has no RCCL; rank 1: it has one device), so
# which is reported, and whether the other got to print, is a race: the case has no record and the test
# asserts only what holds either way.
UNORDERED = ["err_rccl"]
RECORDED = [c for c in CASES if c not in UNORDERED]

SOURCES = [os.path.join(PKG, "csrc", "vbfm_host.cpp"), os.path.join(TESTS, "cli_stub.cpp"),
           os.path.join(TESTS, "cli_stub_model.cpp")]


def build(launcher, exe, extra=()):
    """the compile line of tests/test_host_sanitizers.py; extra: the sanitizer flags, or none. A launcher
    source from elsewhere (another commit's) finds "../../include/vbfm.h" through the second -I"""
    subprocess.run(["g++", "-std=c++17", *extra, "-pthread", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.dirname(LAUNCHER), launcher, *SOURCES, "-o", exe], check=True, capture_output=True, text=True)


_CTIME = re.compile(r"^[A-Z][a-z]{2} [A-Z][a-z]{2} [ \d]\d \d\d:\d\d:\d\d \d{4}$", re.M)
_LOAD_S = re.compile(r'("method": "setup".*?"load_s": )[^,}]+')
_TIMERS = ("time_learn", "time_learn2", "time_learn4")


def _norm_rlog(text):
    lines = text.split("\n")
    head = lines[0].split("\t")
    cols = [i for i, h in enumerate(head) if h in _TIMERS]
    for n in range(1, len(lines)):
        cells = lines[n].split("\t")
        if len(cells) == len(head):
            for i in cols:
                cells[i] = "<t>"
            lines[n] = "\t".join(cells)
    return "\n".join(lines)


def _read(path):
    raw = open(path, "rb").read()
    try:
        return raw.decode("utf-8")
    except UnicodeDecodeError:
        return "hex:" + raw.hex()


def run_case(exe, name, env_extra=None):
    """the record of case `name` run with the launcher `exe`"""
    work = tempfile.mkdtemp(prefix="cli_stub_")
    tr, te = os.path.join(TINY, "train.libfm"), os.path.join(TINY, "test.libfm")
    steps = []
    try:
        for s in CASES[name]:
            flags = list(s["flags"])
            if "-iter" not in flags:
                flags += ["-iter", "3"]
            env = {k: v for k, v in os.environ.items() if not k.startswith(("VBFM_", "ASAN_", "UBSAN_", "LSAN_"))}
            env.update(s["env"], VBFM_STUB_TRACE="trace", **(env_extra or {}))
            r = subprocess.run([exe, "-train", tr, "-test", te, "-dim", "1,1,2", "-seed", "3"] + flags, cwd=work, env=env,
                               capture_output=True, text=True, timeout=120)
            files, traces = {}, {}
            for f in sorted(os.listdir(work)):
                text = _read(os.path.join(work, f))
                if f.startswith("trace."):
                    traces[f[len("trace."):]] = text.splitlines(True)
                    os.remove(os.path.join(work, f))
                elif f == RLOG:
                    files[f] = _norm_rlog(text)
                elif f == "parity.jsonl":
                    files[f] = _LOAD_S.sub(r"\g<1>0", text)
                else:
                    files[f] = text
                if f in files:   # texts as lists of lines: a fixture's diff reads line by line
                    files[f] = files[f].splitlines(True)
            shown = [f.replace(TINY, "tiny") for f in s["flags"]]
            steps.append({"flags": shown, "env": s["env"], "exit": r.returncode, "stdout": _CTIME.sub("<ctime>", r.stdout).splitlines(True),
                          "stderr": r.stderr.splitlines(True), "files": files, "traces": traces})
    finally:
        shutil.rmtree(work)
    return steps


def fixture_path(name):
    return os.path.join(FIXTURES, name + ".json")


def dump(steps):
    return json.dumps(steps, indent=1, sort_keys=True) + "\n"

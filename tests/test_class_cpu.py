"""Binary classification (-task c) without a GPU: the arithmetic of csrc/vbfm_class_math.h and the
reference stream's truncated normals (vbrng::Glibc), compiled for the host in
tests/class_math_check.cpp under ASan + UBSan, against restatements written from the reference's
lines (tests/class_ref.py); the task of a model file; the CLI's task flags."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import class_ref as cr
import vbfm
from conftest import GOLDEN, ROOT, TESTS
from test_host_sanitizers import SAN

PKG = os.path.join(ROOT, "scalable-variational-bayesian-factorization-machine_amd")
CLI = os.path.join(PKG, "bin", "libFM")
TINY = os.path.join(GOLDEN, "tiny")
MUS = (-3.0, -0.5, 0.0, 0.5, 3.0)

needs_gxx = pytest.mark.skipif(not shutil.which("g++"), reason="needs g++")


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("class_math") / "class_math_check")
    subprocess.run(["g++", "-std=c++17", *SAN, "-static-libasan", "-static-libubsan",
                    os.path.join(TESTS, "class_math_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    return exe


def run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe] + [str(a) for a in args], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


@needs_gxx
def test_link_and_expectations_match_the_reference_formulas(check_exe):
    """Phi and the two truncated expectations on x in [-4, 4] to 1e-13 relative (a 1-ulp exp is
    inside that); the same grid is farther than 1e-8 from a libm-erf Phi, so the wrong link fails."""
    g = np.array([[float(v) for v in ln.split()] for ln in run(check_exe, "grid").splitlines()])
    assert g.shape == (801, 4) and g[0, 0] == -4.0 and abs(g[-1, 0] - 4.0) < 1e-12
    x = g[:, 0]
    for col, fn in ((1, cr.Phi), (2, cr.expect_left), (3, cr.expect_right)):
        want = fn(x)
        rel = np.max(np.abs(g[:, col] - want) / np.abs(want))
        print("column", col, "max relative difference", rel)
        assert rel <= 1e-13, (col, rel)
    libm = np.array([0.5 + 0.5 * math.erf(v / math.sqrt(2.0)) for v in x])
    assert np.max(np.abs(g[:, 1] - libm)) > 1e-8


@needs_gxx
@pytest.mark.parametrize("seed", [1, 20261019])
def test_device_mode_sampler_moments(check_exe, seed):
    """1e6 keyed draws at each mean and side: on the target's side of 0, mean and variance within 5
    standard errors of the truncated normal's (a correct sampler fails a check with p ~ 6e-7), no
    row at the attempt cap."""
    rows = [ln.split() for ln in run(check_exe, "sampler", seed).splitlines()]
    assert len(rows) == 10
    for r in rows:
        positive, mu, n = int(r[0]), float(r[1]), int(r[2])
        mean, var, lo, hi = (float(v) for v in r[3:7])
        attempts, capped, nonfinite = int(r[7]), int(r[8]), int(r[9])
        assert capped == 0 and nonfinite == 0 and n <= attempts <= 2.2 * n, r
        if positive:
            assert lo >= 0.0, r
            tm, tv, m4 = cr.trunc_moments(mu)
        else:   # the mirror image: -s is N(-mu, 1) truncated to [0, inf)
            assert hi <= 0.0, r
            tm, tv, m4 = cr.trunc_moments(-mu)
            tm = -tm
        se_mean, se_var = math.sqrt(tv / n), math.sqrt((m4 - tv * tv) / n)
        print(positive, mu, "mean", mean, tm, (mean - tm) / se_mean, "var", var, tv, (var - tv) / se_var)
        assert abs(mean - tm) <= 5 * se_mean, (r, tm)
        assert abs(var - tv) <= 5 * se_var, (r, tv)


@needs_gxx
def test_sampler_cannot_spin(check_exe):
    """A NaN or +-inf yhat returns without one attempt (NaN, flagged); with the cap forced to 0 the
    row takes the truncated expectation (flagged)."""
    lines = [ln.split() for ln in run(check_exe, "edge").splitlines()]
    nonfinite = [l for l in lines if l[0] == "nonfinite"]
    cap0 = [l for l in lines if l[0] == "cap0"]
    assert len(nonfinite) == 6 and len(cap0) == 10
    for l in nonfinite:
        assert (int(l[2]), int(l[3]), int(l[4])) == (0, 1, 1), l   # attempts, CLASS_NONFINITE, is NaN
    for l in cap0:
        side, mu, attempts, flag, s, want = int(l[1]), float(l[2]), int(l[3]), int(l[4]), float(l[5]), float(l[6])
        assert attempts == 0 and flag == 2 and s == want, l
        ref = cr.expect_left(mu) if side == 0 else cr.expect_right(mu)
        assert abs(s - ref) <= 1e-13 * abs(ref), l


class _Stream:
    """The draw loops of random.h:72-114, 150-180 on a given list of uniforms."""

    def __init__(self, u):
        self.u, self.i = u, 0

    def uniform(self):
        v = self.u[self.i]
        self.i += 1
        return v

    def gaussian(self):   # Leva, random.h:150-164
        while True:
            u = self.uniform()
            while u == 0.0:
                u = self.uniform()
            v = 1.7156 * (self.uniform() - 0.5)
            x = u - 0.449871
            y = abs(v) + 0.386595
            q = x * x + y * (0.19600 * y - 0.25472 * x)
            if q < 0.27597:
                return v / u
            if q > 0.27846 or v * v > -4.0 * u * u * math.log(u):
                continue
            return v / u

    def left(self, left):   # random.h:72-102
        if left <= 0.0:
            while True:
                r = self.gaussian()
                if not r < left:
                    return r
        a = 0.5 * (left + math.sqrt(left * left + 4.0))
        while True:
            z = -math.log(1 - self.uniform()) / a + left
            d = z - a
            d = math.exp(-(d * d) / 2)
            if self.uniform() < d:
                return z


@needs_gxx
@pytest.mark.parametrize("mu", [1.0, -1.0])
def test_reference_stream_truncated_normals(check_exe, mu):
    """vbrng::Glibc::left_tgaussian / right_tgaussian: 1000 draws each on their side of 0, equal to
    the restated loops on the same uniforms, and the stream has advanced by exactly the rand() calls
    those loops made (the next uniform is the one the restatement would take next)."""
    out = run(check_exe, "glibc", 12345, mu).splitlines()
    draws = [float(l.split()[1]) for l in out if l.startswith("draw ")]
    rdraws = [float(l.split()[1]) for l in out if l.startswith("rdraw ")]
    nxt = [float(l.split()[1]) for l in out if l.startswith("next ")]
    u = [float(l.split()[1]) for l in out if l.startswith("u ")]
    assert len(draws) == 1000 and len(rdraws) == 1000 and len(nxt) == 1 and len(u) == 40000
    assert min(draws) >= 0.0 and max(rdraws) <= 0.0
    s = _Stream(u)
    for d in draws:   # mean + 1 * left((0 - mean) / 1)
        want = mu + 1.0 * s.left((0.0 - mu) / 1.0)
        assert abs(d - want) <= 1e-14 * max(1.0, abs(want)), (d, want)
    for d in rdraws:  # mean + 1 * -left(-((0 - mean) / 1))
        want = mu + 1.0 * -s.left(-((0.0 - mu) / 1.0))
        assert abs(d - want) <= 1e-14 * max(1.0, abs(want)), (d, want)
    assert s.i >= 2000 and u[s.i] == nxt[0], (s.i, u[s.i], nxt[0])


# ---- the task of a model file ------------------------------------------------------------------
D, K = 7, 2


def _mc_model(rng):
    info = {"kind": 2, "k0": 1, "k1": 1, "num_factor": K, "num_attribute": D, "min_target": -1.0, "max_target": 1.0,
            "iter": 3, "w0_or_mu0": 0.25, "sigma_0_dash": 0.0, "alpha": 1.0}
    return info, {"w": rng.standard_normal(D), "v": rng.standard_normal(K * D)}


def test_model_task_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    info, p = _mc_model(rng)
    pc, pr = str(tmp_path / "c.vbfm"), str(tmp_path / "r.vbfm")
    vbfm.Model.write_params(pc, info, p, task="c")
    vbfm.Model.write_params(pr, info, p)                      # the entry point from before the task existed
    assert vbfm.Model.file_task(pc) == "c" and vbfm.Model.file_task(pr) == "r"
    for path in (pc, pr):
        back = vbfm.Model.read_params(path)
        assert back["w"].tobytes() == p["w"].tobytes() and back["v"].tobytes() == p["v"].tobytes()
        assert back["w0"] == info["w0_or_mu0"]
    hc, hr = open(pc, "rb").read(88), open(pr, "rb").read(88)
    # version 1 / reserved word 0 for regression as ever; version 3 / task 1 for classification, so
    # that a library from before the task existed (it reads version 1 only) refuses the file
    assert struct.unpack("<I", hr[8:12])[0] == 1 and struct.unpack("<I", hr[44:48])[0] == 0
    assert struct.unpack("<I", hc[8:12])[0] == 3 and struct.unpack("<I", hc[44:48])[0] == 1
    assert open(pc, "rb").read()[88:] == open(pr, "rb").read()[88:]


def test_model_file_with_unknown_task_or_kind_is_refused(tmp_path):
    rng = np.random.default_rng(4)
    info, p = _mc_model(rng)
    path = str(tmp_path / "c.vbfm")
    vbfm.Model.write_params(path, info, p, task="c")
    b = bytearray(open(path, "rb").read())
    b[44:48] = struct.pack("<I", 5)
    open(path, "wb").write(bytes(b))
    with pytest.raises(vbfm.VbfmError, match="unknown task"):
        vbfm.Model.file_task(path)
    with pytest.raises(vbfm.VbfmError, match="unknown task"):
        vbfm.Model.read_params(path)
    # a version-1 file keeps ignoring the word (it was reserved): task r
    b[8:12] = struct.pack("<I", 1)
    open(path, "wb").write(bytes(b))
    assert vbfm.Model.file_task(path) == "r"
    # task c belongs to the ALS / MCMC kinds
    vinfo = dict(info, kind=0, sigma_0_dash=0.02)
    vp = {n: rng.standard_normal(s) for n, s in (("mu_w", D), ("sigma_w", D), ("mu_v", K * D), ("sigma_v", K * D))}
    with pytest.raises(vbfm.VbfmError, match="ALS / MCMC kinds only"):
        vbfm.Model.write_params(str(tmp_path / "v.vbfm"), vinfo, vp, task="c")


# ---- CLI flags (no HIP call on these paths) ----------------------------------------------------
def _cli(tmp_path, task, method, *flags):
    return subprocess.run([CLI, "-task", task, "-train", os.path.join(TINY, "train.libfm"), "-test",
                           os.path.join(TINY, "test.libfm"), "-method", method, "-dim", "1,1,2"] + list(flags),
                          cwd=str(tmp_path), capture_output=True, text=True, timeout=120)


@pytest.mark.skipif(not os.path.exists(CLI), reason="bin/libFM not built")
def test_cli_task_flags(tmp_path):
    for method in ("vb", "vb_online"):
        r = _cli(tmp_path, "c", method, "-plan", "1")
        assert "ERROR: task c (binary classification) is provided by the mcmc and als learners" in r.stderr, r.stderr
        assert "Loading train" not in r.stdout and "{" not in r.stdout      # refused before the data load
    for method in ("mcmc", "als"):
        r = _cli(tmp_path, "c", method, "-plan", "1")
        assert "ERROR" not in r.stderr and '"method": "%s"' % method in r.stdout, r.stdout + r.stderr
    r = _cli(tmp_path, "c", "mcmc", "-plan", "1", "-devices", "2", "-transport", "host")
    assert "ERROR" not in r.stderr and r.stdout.count('"rank"') == 2, r.stdout + r.stderr
    r = _cli(tmp_path, "x", "mcmc", "-plan", "1")
    assert "ERROR: unknown task" in r.stderr

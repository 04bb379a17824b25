"""The chain ranking without a GPU: what entitles tests/test_recommend_chain_gpu.py to its conditions. The
case table's share of pairs on the loose sqrt(tol_v) branch of tol_key, computed with a plain numpy FM on
each case's own draws and rows (so the GPU test's 5 % cap can fail only because of the code under test);
the shifted moments of include/vbfm.h "ranking a chain of draws" against np.mean / np.var on adversarial
inputs; and the bindings of the two new symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import vbfm
from conftest import ROOT
from recommend_cases import candidates, contexts
from recommend_chain_cases import (CASE_IDS, CASES, CHAIN_CTX, CHAIN_TILE_B, LOOSE_SHARE, REC_STEP, chain_draws, noise_term,
                                   numpy_raw, shifted_moments, tolerances)


def test_the_case_table_covers_what_the_issue_lists():
    col = lambda i: {c[i] for c in CASES}
    assert col(0) >= {0, 1, 7, 8, 9, 16, 33, 64, 65, 100}
    assert col(3) >= {1, 2, 3, 9, 17}
    assert col(4) >= {CHAIN_CTX - 1, CHAIN_CTX, CHAIN_CTX + 1, CHAIN_TILE_B - 1, CHAIN_TILE_B, CHAIN_TILE_B + 1}
    assert col(5) >= {REC_STEP - 1, REC_STEP, REC_STEP + 1, 2 * REC_STEP + 1} and any(c[5] < c[6] for c in CASES)
    assert col(6) >= {1, 10, 64, 100, 128}
    assert col(7) >= {0.0, 2.0, -1.0, 0.5} and col(8) == {0, 1}
    assert sum(c[9] == "c" for c in CASES) >= 2 and all(c[8] == 0 for c in CASES if c[9] == "c")
    assert all(c[4] <= 65 and c[5] <= 385 and c[3] <= 17 and c[0] <= 100 for c in CASES)


@pytest.mark.parametrize("case", [c for c in CASES if c[3] >= 2], ids=[i for i, c in zip(CASE_IDS, CASES) if c[3] >= 2])
def test_few_pairs_of_a_case_have_a_spread_near_zero(case):
    k, k0, k1, S, B, M, topn, beta, noise, task = case
    draws = chain_draws(k, S)
    raw = numpy_raw(draws, k, k0, k1, contexts(B), candidates(M))
    mean, var = raw.mean(axis=0), raw.var(axis=0)
    loose = tolerances(mean, var, noise_term(draws, noise), beta)[3]
    print("k=%d S=%d B=%d M=%d noise=%d: %.2f %% of %d pairs on the loose branch" % (k, S, B, M, noise, 100 * loose.mean(), loose.size))
    assert loose.mean() <= LOOSE_SHARE


@pytest.mark.parametrize("S", [2, 3, 5, 9, 17, 33, 64])
def test_shifted_moments_agree_with_numpy(S):
    rng = np.random.default_rng(S)
    worst = 0.0
    for level, spread in ((1e3, 1e-3), (1.0, 1.0), (-1e3, 1e-3), (1e3, 10.0)):
        raw = level + spread * rng.standard_normal((S, 2000))
        mean, var = shifted_moments(raw)
        rm, rv = raw.mean(axis=0), raw.var(axis=0)
        # the mean relative to the values it averages (it may itself be near zero), var relative to var
        assert np.all(np.abs(mean - rm) <= 1e-12 * np.max(np.abs(raw), axis=0))
        assert np.all(np.abs(var - rv) <= 1e-12 * rv + 1e-30), (S, level, spread, float(np.max(np.abs(var - rv) / rv)))
        worst = max(worst, float(np.max(np.abs(var - rv) / rv)))
    print("S=%d: worst relative difference of var %.3e" % (S, worst))
    same = np.repeat(rng.standard_normal((1, 100)) * 1e3, S, axis=0)           # all draws equal
    mean, var = shifted_moments(same)
    assert np.array_equal(mean, same[0]) and np.all(var == 0.0)
    one = shifted_moments(same[:1])                                            # S = 1
    assert np.array_equal(one[0], same[0]) and np.all(one[1] == 0.0)


def test_the_bindings_expose_both_symbols():
    assert "vbfm_candidates_create_chain" in vbfm.EXPORTS and "vbfm_recommend_chain" in vbfm.EXPORTS
    with open(os.path.join(ROOT, "include", "vbfm.h")) as fh:
        header = fh.read()
    proto = re.search(r"int vbfm_recommend_chain\(([^;]*)\);", header).group(1)
    assert [a.split()[-1].lstrip("*") for a in proto.split(",")] == ["m", "c", "contexts", "excl_ptr", "excl_idx", "o", "idx", "key",
                                                                      "score", "var", "count", "st"]
    assert re.search(r"int vbfm_candidates_create_chain\(vbfm_candidates \*\*out, vbfm_model \*m, const vbfm_csr \*rows, "
                     r"int32_t unknown_ids\);", header)
    opts = re.search(r"typedef struct \{([^}]*)\} vbfm_recommend_chain_opts;", header).group(1)
    fields = re.findall(r"(int32_t|uint64_t|double) (\w+);", opts)
    assert fields == [("int32_t", "topn"), ("int32_t", "clip"), ("int32_t", "unknown_ids"), ("uint64_t", "chunk_bytes"),
                      ("double", "beta"), ("int32_t", "noise")]
    ctype = {"int32_t": C.c_int32, "uint64_t": C.c_uint64, "double": C.c_double}
    assert [(n, t) for n, t in vbfm.RecommendChainOpts._fields_] == [(n, ctype[t]) for t, n in fields]
    L = vbfm.lib()
    V, P = C.c_void_p, C.POINTER
    assert L.vbfm_candidates_create_chain.argtypes == [P(V), V, P(vbfm.Csr), C.c_int32]
    assert L.vbfm_recommend_chain.argtypes == [V, V, P(vbfm.Csr), vbfm.P_u64, vbfm.P_u32, P(vbfm.RecommendChainOpts), P(C.c_int32),
                                               vbfm.P_f64, vbfm.P_f64, vbfm.P_f64, vbfm.P_u32, P(vbfm.RecommendStats)]
    import inspect
    sig = inspect.signature(vbfm.Model.recommend_chain)
    assert list(sig.parameters) == ["self", "contexts", "candidates", "topn", "beta", "noise", "exclude", "clip", "unknown_ids",
                                    "chunk_bytes"]
    assert sig.parameters["beta"].default == 0.0 and sig.parameters["noise"].default is False
    assert list(inspect.signature(vbfm.Model.candidates_chain).parameters) == ["self", "data", "unknown_ids"]

"""A context gives its device memory back when it is destroyed (vbfm_destroy: store_release,
csrc/vbfm_store.hip, and the other groups' releases). The deferred split's payload -- 8 B per
train entry here, every x being 1 -- is a build product of the store that only the store's own
release knows; a destroy that freed a list of its own leaked it on every create / destroy cycle.

One cycle: create, train and test set, init caches, one iteration, close. After a warm-up cycle
(code objects, the runtime's first-use pools) four more cycles may not lower the device's free
memory by as much as one payload; four leaked payloads are at least four times that.
VBFM_FORCE_SPLIT=1 builds the split forms on one rank, VBFM_PLACE=0 keeps the placement search
(and its transient buffers) out."""
import pytest
import torch

import vbfm

pytestmark = pytest.mark.gpu

N_ROWS, FIELDS, IDS, K = 200_000, 6, 400, 2
PAYLOAD = N_ROWS * FIELDS * 8   # nnz x 8 B


def _cycle(learner, layout):
    D = FIELDS * IDS + 1
    if learner == "vb":
        g = vbfm.FMLearnVB(1, 1, K, D, layout=layout)
    else:
        g = vbfm.FMLearnMCMC(1, 1, K, D, method="mcmc", layout=layout)
    try:
        g.init_device(7)
        g.synth(0, N_ROWS, FIELDS, IDS, 41)
        g.synth(1, 1000, FIELDS, IDS, 42)
        g.init_caches()
        g.iterate()
        assert g.layout() == layout
    finally:
        g.close()


@pytest.mark.parametrize("layout", ["level", "entry"])
@pytest.mark.parametrize("learner", ["vb", "mcmc"])
def test_destroy_returns_device_memory(monkeypatch, learner, layout):
    for kk in ("VBFM_LAYOUT", "VBFM_DEFER", "VBFM_ESTORE", "VBFM_FAULT"):
        monkeypatch.delenv(kk, raising=False)
    monkeypatch.setenv("VBFM_FORCE_SPLIT", "1")
    monkeypatch.setenv("VBFM_PLACE", "0")
    if layout == "entry":
        monkeypatch.setenv("VBFM_DEFER", "1")   # the entry store's split is two-pass unless asked
    _cycle(learner, layout)
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(4):
        _cycle(learner, layout)
    drop = free0 - torch.cuda.mem_get_info()[0]
    print("free memory drop over 4 cycles: %d B = %.2f payloads" % (drop, drop / PAYLOAD))
    assert drop < PAYLOAD

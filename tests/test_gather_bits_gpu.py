"""pdr_gather_add* / pdr_gather_moments* (csrc/fused_gather.hip) against RECORDED bits: tests/golden/gather_bits.npz,
written by tests/golden/make_gather_bits.py from the kernels as they were when the two families still had a device
body each.  test_gather_moments_gpu.py compares the windows against the whole width -- two launches of one body -- so
this file is the comparison against an independent implementation: every moment torch.equal to the fixture (raw
float32), every Y / Yd equal by SHA-256, and every entry the contract leaves unwritten (the residual window of a
moments call, the rows of skipped tiles, the columns behind a Y window) still the sentinel the output was filled with.

Shapes (B = 2, the smallest that reach every path; see CASES in the recipe): 16 / 32 / 64 lanes per row, one and two
column passes, K = 6 (no power of two), the K = 32 ball form with a shared query row and empty balls, and K = 4 below
DEPTH x rows per instruction (a V row per row)."""
import numpy as np
import pytest
import torch

from tests.golden import make_gather_bits as G

from point_diffusion_refinement_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with np.load(G.FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("cid", [c[0] for c in G.CASES])
def test_bits_are_the_recorded_ones(cuda, recorded, cid):
    c, out = G.run_case(_lib.load(), cuda, cid, torch.cuda.current_stream().cuda_stream)
    want = {k.split("/", 1)[1]: v for k, v in recorded.items() if k.startswith(cid + "/")}
    assert sorted(want) == sorted(out), "the fixture and the calls made here differ: re-read the recipe"
    assert len(out) == (15 if cid == G.TILES_CASE else 7)
    G.check_unwritten(c, out)
    for k, v in sorted(out.items()):
        if k.endswith(".moments"):
            assert torch.equal(v.cpu(), torch.from_numpy(want[k])), "%s: moments differ from the recorded bits" % k
        else:
            assert np.array_equal(G.digest(v), want[k]), "%s: bytes differ from the recorded ones" % k

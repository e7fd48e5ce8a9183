"""CPU: the fp32 oracle (oracle/gsrast_oracle.c) against numbers the REFERENCE's own kernels wrote -- tests/golden/ref_kernel_vectors.npz,
recorded on the MI355X from oracle/_ref/libref_rasterizer.so (oracle/ref_build.py; tests/golden/make_golden.py refkernels) for three of
the edge cases: white background on a 50 x 37 image, precomputed colours + covariances, scale_modifier 0.7.

The comparisons are those of tests/test_gpu_reference_kernels.py (ref_compare): (a) the recorded outputs and gradients against the fp64
math renderer, (b) the oracle's per-Gaussian arrays, tile counts, sorted keys, point list and tile ranges against the recorded ones.  So a
change to the oracle -- or an error it shares with csrc/gsrast_preprocess.h, which every -m gpu test would then share too -- is checked
against the reference's kernels on every machine.  Regenerating the file on the MI355X is the only way to change it."""
import json
import os
import sys

import numpy as np
import pytest

import ref_compare as rc
import ref_kernels

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_golden import input_digest      # noqa: E402

ARRAYS = ref_kernels.FORWARD_OUT + ref_kernels.BACKWARD_OUT + ("present",)


@pytest.fixture(scope="module")
def recorded():
    z = np.load(os.path.join(HERE, "golden", "ref_kernel_vectors.npz"))
    assert tuple(z["names"]) == rc.GOLDEN_CASES
    return z, ref_kernels.unpack(z, list(rc.GOLDEN_CASES))


@pytest.mark.parametrize("name", rc.GOLDEN_CASES)
def test_the_inputs_regenerate(name, recorded):
    """The fixture stores no inputs: the case built from its seeds today must be the one the kernels ran on."""
    rb, t = recorded[1][name], rc.truth(name)
    assert set(ARRAYS) <= set(rb)
    assert int(rb["g_seed"]) == t["r"]["g_seed"]
    packed = ref_kernels.pack_case(name, t["r"]["sc"], t["r"]["cam"], t["c"]["deg"], t["r"]["g"])
    assert input_digest(packed, name) == str(rb["input_sha256"]), "the case's generator drifted: regenerate the fixture on the MI355X"


@pytest.mark.parametrize("name", rc.GOLDEN_CASES)
def test_recorded_reference_kernels_against_the_fp64_math_renderer(name, recorded):
    rc.check_truth(name, recorded[1][name], "recorded reference binary")


@pytest.mark.parametrize("name", rc.GOLDEN_CASES)
def test_oracle_intermediates_and_lists_against_the_recorded_reference_kernels(name, recorded):
    rb, t = recorded[1][name], rc.truth(name)
    rc.check_intermediates(name, rb)
    rc.check_lists(name, rb, t["o32"], "fp32 oracle")
    from oracle import oracle as orc
    np.testing.assert_array_equal(np.asarray(rb["present"]) != 0, orc.mark_visible(t["r"]["sc"]["means3D"], t["r"]["cam"]["viewmatrix"], t["r"]["cam"]["projmatrix"]))


def test_oracle_gradients_sit_with_the_recorded_reference_kernels(recorded):
    """The gradient bar's premise (conftest.grad_tol): the fp32 oracle is the reference's fp32 floor.  The recorded reference gradients need
    well under the 8 x of the bar, and the oracle's own error is of the same size: neither side more than 8 x the other, per tensor."""
    for name in rc.GOLDEN_CASES:
        rb, t = recorded[1][name], rc.truth(name)
        r = t["r"]
        ref = rc.grads_by_leaf(r, rb)
        for n in r["names"] + ["means2D"]:
            e_ref, e_orc = float(np.abs(ref[n] - r["want"][n]).max()), float(np.abs(t["f32"][n] - r["want"][n]).max())
            print(f"{name}: {n}: max |refbin - truth| {e_ref:.3e}   max |oracle32 - truth| {e_orc:.3e}")
            assert e_ref <= 8.0 * e_orc and e_orc <= 8.0 * e_ref, (name, n, e_ref, e_orc)


def test_recorded_source_hashes_match_the_built_library(recorded):
    """When oracle/_ref/ is there, it must have been compiled from the sources the fixture was recorded with."""
    z = recorded[0]
    want = dict(zip((str(k) for k in z["source_files"]), (str(v) for v in z["source_sha256"])))
    assert {"forward.cu", "backward.cu", "rasterizer_impl.cu"} <= set(want)
    manifest = os.path.join(os.path.dirname(ref_kernels.LIB_PATH), "manifest.json")
    if os.path.exists(manifest):
        with open(manifest) as f:
            assert json.load(f)["sources"] == want

"""The adversarial families of tests/edge_families.py through the HIP path, judged directly by the second restatement
(oracle/pyref.py, written from the Rust text) as well as by the C oracle -- so that a misreading shared by the oracle and the
kernels that were tuned against it cannot stay green.

(a) every 3-D family on every parity tap (leaf indices, patch flags, both guess grids, the guesses, both accumulators, both
    mean-shift traces, the pose), on the uniform path and with DH_FORCE_GENERAL=1;
(b) the sibling consumers at their limits (k_mask, k_hough2d + k_narrow_u16, k_blur_u16, k_argmax2d): vote sums past 65 535,
    the valtoadd limits, stride squares clipped at every border, blur kernels longer than the frame, frame widths around the
    256-thread blur tile, a saturating blur, argmax ties and depth-0 winners -- several frames per call throughout."""
import os

import numpy as np
import pytest

import edge_families as ef
from test_edge_pyref import KEYS, aux_family_results, family_results

pytestmark = pytest.mark.gpu

# Families whose forests the reference runs but dh_forest_create refuses (depthhead_amd/csrc/dh_host.cpp), with the refusal's
# message.  NaN thresholds: `avg1 - avg2 > NaN` is false for every window (houghforest.rs:185-193), the same as `> +inf`,
# but the kernels' split tests assume an ordered threshold.  Non-finite rotations: the refusal checks every rotation's bin,
# while the reference computes bins only for leaves that pass the covariance gate (prediction.rs:600), which a non-finite
# rotation never does.  Both refusals guard kernel indexing; accepting these forests is left to a change of its own.
REFUSED = {"nonfinite_thresholds": "NaN threshold", "nonfinite_rotations": "rotation bin"}


@pytest.fixture(scope="module")
def hp_mod(hip_lib):
    from depthhead_amd import prediction
    return prediction


class general_path:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        if self.on:
            os.environ["DH_FORCE_GENERAL"] = "1"

    def __exit__(self, *exc):
        os.environ.pop("DH_FORCE_GENERAL", None)


def _hip_taps(hp_mod, fam):
    n, h, w = fam.frames.shape
    with hp_mod.HoughPrediction(fam.forest, fam.model, device=0) as hp:
        hp.debug_enable(True)
        poses = hp.predict_batch(fam.frames, hp_mod.IntrinsicMatrix(fam.K), fam.midp, fam.rot)
        leaf, flags = hp.debug_leaf_indices(n, w, h), hp.debug_patch_flags(n, w, h)
        pos_grid, rot_grid = hp.debug_grids(n)
        guesses = hp.debug_guesses(n)
        tr_mid, st_mid = hp.debug_meanshift(n, 0)
        tr_rot, st_rot = hp.debug_meanshift(n, 1)
        votes = [(hp_mod.aggregate_votes(hp.debug_votes(i, 0)), hp_mod.aggregate_votes(hp.debug_votes(i, 1))) for i in range(n)]
    return [dict(leaf_idx=leaf[i], patch_flags=flags[i], pos_grid=pos_grid[i], rot_grid=rot_grid[i], guess_mid=guesses[i, :3],
                 guess_rot=guesses[i, 3:], mid_cells=votes[i][0], rot_cells=votes[i][1], ms_trace_mid=(tr_mid[i], st_mid[i]),
                 ms_trace_rot=(tr_rot[i], st_rot[i]), mid_point=poses["mid_point"][i], rotation=poses["rotation"][i])
            for i in range(n)]


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("name", list(ef.FAMILIES))
def test_hip_against_pyref(hp_mod, name, general):
    fam, res = family_results(name)
    if name in REFUSED:
        # KNOWN DIVERGENCES, not fixed here: the reference runs these forests, dh_forest_create refuses them (see REFUSED)
        from depthhead_amd._lib import DepthheadError
        with pytest.raises(DepthheadError, match=REFUSED[name]):
            hp_mod.HoughPrediction(fam.forest, fam.model, device=0)
        return
    with general_path(general):
        got = _hip_taps(hp_mod, fam)
    it = fam.model.meanshift_iterations
    for i, (g, r) in enumerate(zip(got, res)):
        for k in KEYS:
            if k.startswith("ms_trace"):
                tr, st = g[k]
                n = r[k].shape[0]                     # pyref's steps + 1
                # the kernel stops at a fixed point and reports the remaining (identical) steps as done
                assert st + 1 >= n or st == it, (name, i, k, st, n)
                assert np.array_equal(tr[:n], r[k]), (name, i, k, tr[:n], r[k])
            else:
                assert np.array_equal(g[k], r[k]), (name, i, k, g[k], r[k])


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("name", list(ef.AUX_FAMILIES))
def test_hip_aux_limits(hp_mod, oracle, name, general):
    fam, res = aux_family_results(name)
    K = hp_mod.IntrinsicMatrix(fam.K)
    with general_path(general):
        with hp_mod.HoughPrediction(fam.forest, fam.model, device=0) as hp:
            masks = hp.predict_mask(fam.frames)
            votes = hp.build_hough_votes(fam.frames, K)
            blurred = hp.build_hough_image(fam.frames, K)
            poses = hp.predict_parameter_from2dhough(fam.frames, K)
    sigma = fam.model.gaussian_sigma
    for i, f in enumerate(fam.frames):
        assert np.array_equal(masks[i], res[i]["mask"]), (name, i)
        assert np.array_equal(masks[i], oracle.predict_mask(fam.forest, fam.model, f)), (name, i)
        assert np.array_equal(votes[i], res[i]["votes"]), (name, i)
        assert np.array_equal(votes[i], oracle.hough_image(fam.forest, fam.model, f, fam.K)), (name, i)
        assert np.array_equal(blurred[i], oracle.gaussian_blur_u16(res[i]["votes"], sigma)), (name, i)
        assert np.array_equal(blurred[i], oracle.build_hough_image(fam.forest, fam.model, f, fam.K)), (name, i)
        mid, rot = oracle.predict_from2dhough(fam.forest, fam.model, f, fam.K)
        assert np.array_equal(poses["mid_point"][i], mid) and np.all(poses["rotation"][i] == 0.0), (name, i, poses[i], mid)
    ef.expectations(fam, blurred, fam.frames)          # the kernels' own images reach the family's edge

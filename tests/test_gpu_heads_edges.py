"""Several heads per frame on the GPU at the edges of the definition: dh_predict_heads and its camera / device twins byte for
byte (n_heads and every dh_head of every slot) against the restatement of tests/heads_ref.py, on the placed scenes of
tests/heads_scenes.py and the adversarial families of tests/edge_families.py.

(a) every placed scene on both traversal paths, at every max_heads and radius it lists: the host call, the camera call with
    the scene's frames seen once through their own K and once through a mixed pinhole / general decoy table, and both
    `_device` forms between guard bands; the scene's `reach` on the kernels' own records;
(b) every 3-D family the same way, with its own K and with its decoy cameras, at max_heads 4 and the radii 0,
    DH_SUPPORT_RADIUS, 2^31 - 1, r*, r* - 1; the forests dh_forest_create refuses are refused here as well;
(c) launch shapes on placed frames: each frame alone; 65 frames (the second workgroup of k_heads_finish with one live
    thread); 2049 frames with the tree set doubled (hd_grid gives one workgroup per frame, and the grid-stride loops of
    k_heads_moments and k_heads_support make a second pass), in a child process; one frame with a few thousand hit records
    (many workgroups meet k_heads_support's last-workgroup ticket);
(d) the heads scratch's lifecycle on one predictor: four heads in every frame, then one seed per frame in fewer frames, then
    the first batch at max_heads 2, then a support call and a plain call -- each equal to a fresh predictor's.
"""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_families as ef
import gpu_kit
import heads_scenes as hs
import support_ref as sr
from test_gpu_edge_families import REFUSED, general_path
from test_heads_scenes import from_oracle, scene_results

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HD_THREADS = 256            # k_heads.hip
HB = 80                     # sizeof(dh_head)


@pytest.fixture(scope="module")
def mods(hip_lib):
    from depthhead_amd import _lib, prediction, tracking
    return _lib, prediction, tracking


def hd_grid_x(n_frames, hits_cap):
    """Workgroups per frame of k_heads_moments and k_heads_support (hd_grid, k_heads.hip)."""
    per = (hits_cap + HD_THREADS - 1) // HD_THREADS
    want = (2048 + n_frames - 1) // n_frames
    return max(1, min(per, want))


def same_heads(got, want, what):
    """(n_heads, heads) against (n_heads, heads): the counts, then every record of every slot, the zero ones included."""
    assert np.array_equal(np.asarray(got[0]).reshape(-1), np.asarray(want[0]).reshape(-1)), (what, got[0], want[0])
    gpu_kit.same_records(got[1], want[1], what)


def decoy_table(K, n):
    """One decoy camera per frame: pinhole variants of K on even frames, cameras with a skew term (not pinhole) on odd ones."""
    Ds = np.repeat(np.asarray(K, np.float32)[None], n, axis=0).copy()
    for j in range(n):
        s = 1.0 + 0.03 * (j + 1)
        Ds[j, 0, 0] *= s; Ds[j, 1, 1] /= s; Ds[j, 0, 2] += 2.5 * (j + 1); Ds[j, 1, 2] -= 1.5 * (j + 1)
        if j % 2:
            Ds[j, 0, 1] = 0.5
    assert any(ef.is_pinhole(D) for D in Ds) and (n < 2 or not all(ef.is_pinhole(D) for D in Ds))
    return Ds


def device_call(_lib, P, hp, frames, cam, mh, r, cameras):
    """One `_device` call with the frames, n_heads and heads between guard bands: (n_heads, heads) after checking the bands."""
    import torch
    n, h, w = frames.shape
    ft, whole = gpu_kit.between_guards(frames, 4096, 700)
    nb, nptr, noff = gpu_kit.guarded(n * 4, 4)
    hb, hptr, hoff = gpu_kit.guarded(n * mh * HB, 8)
    s = torch.cuda.current_stream().cuda_stream
    if cameras:
        hp.predict_heads_cameras_device(ft.data_ptr(), n, w, h, cam, nptr, hptr, mh, r, stream=s)
    else:
        hp.predict_heads_device(ft.data_ptr(), n, w, h, cam, nptr, hptr, mh, r, stream=s)
    torch.cuda.synchronize()
    assert gpu_kit.untouched(nb, noff, n * 4) and gpu_kit.untouched(hb, hoff, n * mh * HB), "a guard band was written"
    got_n = nb.cpu().numpy()[noff:noff + n * 4].copy().view(np.uint32)
    got = hb.cpu().numpy()[hoff:hoff + n * mh * HB].copy().view(_lib.HEAD_DTYPE).reshape(n, mh)
    del whole
    return got_n, got


# ---------------------------------------------------------------------------------------------------- (a) the placed scenes
_decoy = {}


def scene_decoys(oracle, name):
    """(decoy cameras, the restatement of the scene's frames seen through them), once per session."""
    if name not in _decoy:
        sc = hs.scene(name)
        Ds = decoy_table(sc.K, len(sc.frames))
        _decoy[name] = (Ds, from_oracle(oracle, sr.LeafTables(sc.forest), sc.model, sc.frames, Ds, sc.runs()))
    return _decoy[name]


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("name", list(hs.SCENES))
def test_placed_scene(mods, oracle, name, general):
    _lib, P, TR = mods
    sc, want, _, _ = scene_results(name)
    Ds, want_decoy = scene_decoys(oracle, name)
    n = len(sc.frames)
    both = np.concatenate([sc.frames, sc.frames])
    Ks = np.concatenate([np.repeat(np.asarray(sc.K, np.float32)[None], n, axis=0), Ds])
    got, got_cam = {}, {}
    with general_path(general):
        with P.HoughPrediction(sc.forest, sc.model, device=0) as hp, TR.Cameras(Ks) as cams:
            for mh, r in sc.runs():
                got[(mh, r)] = hp.predict_heads(sc.frames, P.IntrinsicMatrix(sc.K), mh, r)
                if general:
                    assert hp.debug_geometry()["uniform"] == 0
                got_cam[(mh, r)] = hp.predict_heads_cameras(both, cams, mh, r)
            mh, r = sc.runs()[0]
            dev = device_call(_lib, P, hp, sc.frames, P.IntrinsicMatrix(sc.K), mh, r, False)
            dev_cam = device_call(_lib, P, hp, both, cams, mh, r, True)
    for key in sc.runs():
        same_heads(got[key], want[key], (name, general, key, "predict_heads"))
        same_heads((got_cam[key][0][:n], got_cam[key][1][:n]), want[key], (name, general, key, "cameras, own K"))
        same_heads((got_cam[key][0][n:], got_cam[key][1][n:]), want_decoy[key], (name, general, key, "cameras, decoys"))
    key = sc.runs()[0]
    same_heads(dev, want[key], (name, general, key, "predict_heads_device"))
    same_heads((dev_cam[0][:n], dev_cam[1][:n]), want[key], (name, general, key, "cameras_device, own K"))
    same_heads((dev_cam[0][n:], dev_cam[1][n:]), want_decoy[key], (name, general, key, "cameras_device, decoys"))
    met = sc.reach(got)                                     # the scene's edge on the kernels' own records
    assert met and all(met.values()), met


# ---------------------------------------------------------------------------------------------------- (b) the families
@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("name", list(ef.FAMILIES))
def test_family(mods, name, general):
    _lib, P, TR = mods
    if name in REFUSED:
        fam = ef.FAMILIES[name]()
        with pytest.raises(_lib.DepthheadError, match=REFUSED[name]):      # the refusal of test_gpu_edge_families stands
            P.HoughPrediction(fam.forest, fam.model, device=0)
        return
    for decoy in (False, True):
        fh = hs.family_heads(name, decoy)
        fam, frames = fh["fam"], fh["frames"]
        with general_path(general):
            with P.HoughPrediction(fam.forest, fam.model, device=0) as hp, \
                    (TR.Cameras(fh["Ks"]) if decoy else contextlib.nullcontext()) as cams:
                cam = cams if decoy else P.IntrinsicMatrix(fam.K)
                for mh, r in fh["runs"]:
                    got = hp.predict_heads_cameras(frames, cam, mh, r) if decoy else hp.predict_heads(frames, cam, mh, r)
                    same_heads(got, fh["results"][(mh, r)], (name, general, decoy, r))
                if general:
                    assert hp.debug_geometry()["uniform"] == 0
                mh, r = fh["runs"][3]
                dev = device_call(_lib, P, hp, frames, cam, mh, r, decoy)
        same_heads(dev, fh["results"][(mh, r)], (name, general, decoy, r, "device"))


# ---------------------------------------------------------------------------------------------------- (c) launch shapes
@pytest.mark.parametrize("name", list(hs.SCENES))
def test_each_placed_frame_alone(mods, name):
    _lib, P, _ = mods
    sc, want, _, _ = scene_results(name)
    key = sc.runs()[0]
    with P.HoughPrediction(sc.forest, sc.model, device=0) as hp:
        for i in range(len(sc.frames)):
            got = hp.predict_heads(sc.frames[i:i + 1], P.IntrinsicMatrix(sc.K), *key)
            same_heads(got, (want[key][0][i:i + 1], want[key][1][i:i + 1]), (name, i, "batch of 1"))


def test_65_frames_second_finish_workgroup(mods):
    """65 frames: k_heads_finish runs two workgroups of 64 threads, the second with one live thread -- frame 64, the chain frame."""
    _lib, P, _ = mods
    sc, want, _, _ = scene_results("finish")
    idx = np.random.RandomState(23).randint(0, len(sc.frames), 65)
    idx[64] = 7
    for key in ((4, 12), (1, 12)):
        with P.HoughPrediction(sc.forest, sc.model, device=0) as hp:
            got = hp.predict_heads(sc.frames[idx], P.IntrinsicMatrix(sc.K), *key)
        same_heads(got, (want[key][0][idx], want[key][1][idx]), ("65 frames", key))
    assert want[(4, 12)][0][7] == 2


def doubled_cubes(oracle, frames, runs):
    """(forest of `cubes` with its tree set twice, the restatement of `frames` over it)."""
    sc = hs.scene("cubes")
    forest = hs.more_trees(sc.forest, 2)
    return sc, forest, from_oracle(oracle, sr.LeafTables(forest), sc.model, frames, [sc.K] * len(frames), runs)


def hit_counts(P, forest, model, frames, K):
    with P.HoughPrediction(forest, model, device=0) as hp:
        hp.debug_enable(True)
        hp.predict_batch(frames, P.IntrinsicMatrix(K))
        return hp.debug_hit_counts(len(frames))


_CHILD_2049 = r"""
import sys
import numpy as np
import torch
from depthhead_amd import synth
from depthhead_amd.forest import Forest
from depthhead_amd.prediction import HoughPrediction, IntrinsicMatrix
d = np.load(sys.argv[1])
frames, K, mh, r = d["base"][d["idx"]], d["K"], int(d["mh"]), int(d["r"])
n, h, w = frames.shape
dev = torch.device("cuda", 0)
ft = torch.from_numpy(frames.view(np.int16)).to(dev)
nd = torch.zeros(n, dtype=torch.int32, device=dev)
hd = torch.zeros(n * mh * 80, dtype=torch.uint8, device=dev)
forest = Forest.load(sys.argv[2])
with HoughPrediction(forest, synth.ModelParams(stepwidth=4, subimage_width=8, subimage_height=8)) as hp:
    hp.set_forking(1)
    hp.predict_heads_device(ft.data_ptr(), n, w, h, IntrinsicMatrix(K), nd.data_ptr(), hd.data_ptr(), mh, r,
                            stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
np.savez(sys.argv[3], n_heads=nd.cpu().numpy(), heads=hd.cpu().numpy())
print("child ok")
"""


def test_2049_frames_one_workgroup_per_frame(mods, oracle, tmp_path):
    """2049 frames in one launch (DH_MAX_RESIDENT_FRAMES = 2049, no forking, a fresh child process): hd_grid gives one
    workgroup per frame, which walks a frame of more than 256 hit records in two passes; k_heads_finish's last workgroup
    has one live thread."""
    _lib, P, _ = mods
    n = 2049
    base = hs.cubes_variants()
    key = (4, hs.R_STAR)
    sc, forest, want = doubled_cubes(oracle, base, [key])
    assert sorted(int(v) for v in want[key][0]) == [0, 1, 3, 3, 4], want[key][0]
    nx, ny = sc.model.patch_grid(hs.W, hs.H)
    assert hd_grid_x(n, nx * ny * forest.n_trees) == 1
    hits = hit_counts(P, forest, sc.model, base, sc.K)
    assert hits.max() > HD_THREADS and 0 < hits[3] <= HD_THREADS and hits[2] == 0, hits     # a second pass; one pass; none
    idx = np.random.RandomState(29).randint(0, len(base), n)
    idx[n - 1] = 0
    np.savez(str(tmp_path / "in.npz"), base=base, idx=idx, K=sc.K, mh=key[0], r=key[1])
    forest.save(str(tmp_path / "forest.npz"))
    script = tmp_path / "child.py"
    script.write_text(_CHILD_2049)
    env = dict(os.environ, DH_MAX_RESIDENT_FRAMES=str(n), PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, str(script), str(tmp_path / "in.npz"), str(tmp_path / "forest.npz"),
                          str(tmp_path / "out.npz")], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert res.returncode == 0 and "child ok" in res.stdout, (res.returncode, res.stderr[-3000:])
    got = np.load(tmp_path / "out.npz")
    same_heads((got["n_heads"].view(np.uint32), got["heads"].view(_lib.HEAD_DTYPE).reshape(n, key[0])),
               (want[key][0][idx], want[key][1][idx]), "2049 frames, one workgroup per frame")


def test_one_frame_of_thousands_of_hit_records(mods, oracle):
    """One frame whose flat block gives a few thousand hit records: k_heads_moments and k_heads_support run many workgroups
    on it, and the last of them to finish writes the records and clears the scratch."""
    _lib, P, _ = mods
    frames = hs.cubes_block()
    runs = [(4, hs.R_STAR), (4, hs.R_STAR - 1)]
    sc, forest, want = doubled_cubes(oracle, frames, runs)
    nx, ny = sc.model.patch_grid(hs.W, hs.H)
    gx = hd_grid_x(1, nx * ny * forest.n_trees)
    hits = hit_counts(P, forest, sc.model, frames, sc.K)
    assert gx >= 16 and hits[0] > 2000 and hits[0] > 8 * HD_THREADS, (gx, hits)
    assert want[runs[0]][0][0] >= 2 and hs.differ(want, runs[0], runs[1])
    with P.HoughPrediction(forest, sc.model, device=0) as hp:
        for key in runs:
            for rep in range(2):                            # the second call finds the scratch the first one left
                same_heads(hp.predict_heads(frames, P.IntrinsicMatrix(sc.K), *key), want[key], ("flat block", key, rep))


# ---------------------------------------------------------------------------------------------------- (d) lifecycle
def test_heads_scratch_lifecycle_on_one_predictor(mods):
    """Moments, bitmaps, accumulators and 20^3 grids are zero between calls by construction: a slot that a call leaves
    non-zero shows in the next call that uses fewer heads, fewer frames or another entry point."""
    _lib, P, _ = mods
    sc, want, _, _ = scene_results("seed_order")
    K = P.IntrinsicMatrix(sc.K)
    four = sc.frames[[0, 1, 0, 1, 1, 0, 0, 1]]
    one = sc.frames[[3, 3, 3]]
    w4, w2, w1 = want[(4, 30)], want[(2, 30)], want[(4, 30)]
    sel4, sel1 = [0, 1, 0, 1, 1, 0, 0, 1], [3, 3, 3]
    assert (w4[0][sel4] == 4).all() and (w1[0][sel1] == 1).all()

    def fresh(call):
        with P.HoughPrediction(sc.forest, sc.model, device=0) as hq:
            return call(hq)

    calls = [("1: four heads in every frame", lambda h: h.predict_heads(four, K, 4, 30), (w4[0][sel4], w4[1][sel4])),
             ("2: one seed per frame, fewer frames", lambda h: h.predict_heads(one, K, 4, 30), (w1[0][sel1], w1[1][sel1])),
             ("3: the first batch at max_heads 2", lambda h: h.predict_heads(four, K, 2, 30), (w2[0][sel4], w2[1][sel4])),
             ("4: a support call", lambda h: h.predict_batch_support(four, K, 30), None),
             ("5: a plain call", lambda h: h.predict_batch(four, K), None),
             ("6: four heads again", lambda h: h.predict_heads(four, K, 4, 30), (w4[0][sel4], w4[1][sel4]))]
    with P.HoughPrediction(sc.forest, sc.model, device=0) as hp:
        for what, call, expect in calls:
            got, ref = call(hp), fresh(call)
            got, ref = (got if isinstance(got, tuple) else (got,)), (ref if isinstance(ref, tuple) else (ref,))
            for g, f in zip(got, ref):
                assert g.tobytes() == f.tobytes(), what
            if expect is not None:
                same_heads(got, expect, what)

"""Training of Hough forests on the GPU: the reference's `HoughLearning` (src/hough/prediction.rs:69-234).

`HoughLearning(...).learn(sigma, data)` extracts the training windows of every frame on the device, grows
`num_of_trees` trees breadth-first with one split-search launch per level, and returns an ordinary `Forest` with
the `ModelParams` of the `HoughPrediction` the reference would return (`meanshift_iterations = 20`, :225-233).
What the reference pins is restated exactly; its random draws (`thread_rng`) and stamm's tree growing are
defined by `seed` ("parity unpinned").  All arithmetic runs in libdepthhead_hip.so.
"""
from __future__ import annotations

import ctypes as C
import json

import numpy as np

from . import _lib
from ._lib import check, vp
from .forest import NODE_DTYPE, Forest
from .synth import ModelParams

# frames handed to one dh_trainer_add_frames call by learn(); the pool does not depend on this
_LEARN_BATCH = 64


def export_forest(lib, handle) -> Forest:
    """dh_forest_export: a library-side forest back into numpy arrays."""
    info = [C.c_uint32() for _ in range(4)]
    check(lib.dh_forest_info(handle, *[C.byref(i) for i in info]))
    nt, nn, nl = info[0].value, info[1].value, info[2].value
    n_off, n_rot = C.c_uint32(), C.c_uint32()
    check(lib.dh_forest_export(handle, None, None, None, None, None, None, None, C.byref(n_off), C.byref(n_rot)))
    roots = np.zeros(nt, np.int32)
    nodes = np.zeros(nn, NODE_DTYPE)
    prob = np.zeros(nl, np.float64)
    ob = np.zeros(nl + 1, np.uint32)
    rb = np.zeros(nl + 1, np.uint32)
    offs = np.zeros((n_off.value, 3), np.float32)
    rots = np.zeros((n_rot.value, 3), np.float64)
    check(lib.dh_forest_export(handle, vp(roots), vp(nodes), vp(prob), vp(ob), vp(rb), vp(offs), vp(rots), None, None))
    return Forest(roots, nodes, prob, ob, rb, offs, rots)


class Trainer(_lib._Handle):
    """One dh_trainer: a sample pool on `device` fed by `add_frames`, fitted by `fit` (any number of times)."""
    _handles = (("_h", "dh_trainer_destroy"),)

    def __init__(self, params: "_lib.TrainParams", device: int = 0):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        check(self._lib.dh_trainer_create(C.byref(params), int(device), C.byref(self._h)))

    def add_frames(self, frames, masks, K, pos3d, rot_deg) -> None:
        """frames [n, H, W] u16, masks [n, H, W] (non-zero = head), K [n, 3, 3] or one [3, 3], pos3d / rot_deg [n, 3]."""
        frames = np.ascontiguousarray(frames, dtype=np.uint16)
        if frames.ndim == 2:
            frames = frames[None]
        n, h, w = frames.shape
        masks = np.ascontiguousarray(np.asarray(masks).reshape(n, h, w) != 0, dtype=np.uint8)
        K = np.asarray(K, dtype=np.float32)
        K = np.ascontiguousarray(np.broadcast_to(K.reshape(-1, 9), (n, 9)) if K.size == 9 else K.reshape(n, 9))
        p3 = np.ascontiguousarray(pos3d, dtype=np.float32).reshape(n, 3)
        rd = np.ascontiguousarray(rot_deg, dtype=np.float32).reshape(n, 3)
        check(self._lib.dh_trainer_add_frames(self._h, vp(frames), vp(masks), n, w, h, vp(K), vp(p3), vp(rd)))

    def fit(self) -> Forest:
        f = C.c_void_p()
        check(self._lib.dh_trainer_fit(self._h, C.byref(f)))
        try:
            return export_forest(self._lib, f)
        finally:
            self._lib.dh_forest_destroy(f)

    def stats(self, cap_levels: int = 64) -> dict:
        st = _lib.TrainStats()
        nodes, leaves = np.zeros(cap_levels, np.uint32), np.zeros(cap_levels, np.uint32)
        ms = np.zeros(cap_levels, np.float32)
        check(self._lib.dh_trainer_stats(self._h, C.byref(st), vp(nodes), vp(leaves), vp(ms), cap_levels))
        L = min(st.levels, cap_levels)
        return {"frames": st.frames, "pool_size": st.pool_size, "pool_positives": st.pool_positives, "neg_det": st.neg_det,
                "levels": st.levels, "nodes_per_level": nodes[:L].tolist(), "leaves_per_level": leaves[:L].tolist(),
                "level_ms": [float(x) for x in ms[:L]]}


class HoughLearning:
    """prediction.rs:69-143.  Arguments in the reference's order; `seed` keys every random draw, `device` is the GPU."""

    def __init__(self, stepwidth, subimg_width, subimg_height, max_depth, num_of_trees, subset_size_per_tree,
                 subrect_feature_scale, feature_number_per_node, min_subset_size_to_stop, steepness_weighting,
                 seed: int = 0, device: int = 0):
        s = float(subrect_feature_scale)
        ints = dict(stepwidth=stepwidth, subimg_width=subimg_width, subimg_height=subimg_height, max_depth=max_depth,
                    num_of_trees=num_of_trees, subset_size_per_tree=subset_size_per_tree,
                    feature_number_per_node=feature_number_per_node, min_subset_size_to_stop=min_subset_size_to_stop)
        for name, v in ints.items():   # u32 / usize in the reference: a negative value would wrap in the C structure
            if int(v) != v or not 0 <= int(v) <= 0xFFFFFFFF:
                raise ValueError(f"{name} = {v} is not an unsigned 32-bit integer")
        # HoughLearning::new returns None exactly here (HoughTreeFunctions::new, houghforest.rs:149-153); a factor of 0
        # passes `new` there but panics at the first node (random_subrect_iterator(..).unwrap(), types.rs:106-109)
        if not (0.0 < s <= 1.0):
            raise ValueError(f"subrect_feature_scale {s} outside (0, 1]")
        if int(feature_number_per_node) == 0:
            raise ValueError("feature_number_per_node must be > 0")
        if not (float(steepness_weighting) > 0.0):
            raise ValueError("steepness_weighting must be > 0")
        self.stepwidth = int(stepwidth)
        self.subimg_width, self.subimg_height = int(subimg_width), int(subimg_height)
        self.max_depth, self.num_of_trees = int(max_depth), int(num_of_trees)
        self.subset_size_per_tree = int(subset_size_per_tree)
        self.subrect_feature_scale = s
        self.feature_number_per_node = int(feature_number_per_node)
        self.min_subset_size_to_stop = int(min_subset_size_to_stop)
        self.steepness_weighting = float(steepness_weighting)
        self.seed, self.device = int(seed), int(device)
        self.last_stats: dict | None = None

    def params(self) -> "_lib.TrainParams":
        return _lib.TrainParams(self.stepwidth, self.subimg_width, self.subimg_height, self.max_depth, self.num_of_trees,
                                self.subset_size_per_tree, self.subrect_feature_scale, self.feature_number_per_node,
                                self.min_subset_size_to_stop, self.steepness_weighting, self.seed & 0xFFFFFFFFFFFFFFFF)

    def trainer(self) -> Trainer:
        return Trainer(self.params(), self.device)

    def learn(self, gaussian_sigma: float, data) -> tuple[Forest, ModelParams]:
        """`data` yields (depth [H, W] u16, mask [H, W], K [3, 3], pos3d [3] mm, rot_deg [3]).  Consecutive frames of
        one size are uploaded together."""
        with self.trainer() as tr:
            batch: list = []

            def flush():
                if batch:
                    tr.add_frames(np.stack([b[0] for b in batch]), np.stack([b[1] for b in batch]),
                                  np.stack([np.asarray(b[2], np.float32).reshape(9) for b in batch]),
                                  np.stack([b[3] for b in batch]), np.stack([b[4] for b in batch]))
                    batch.clear()

            for item in data:
                depth = np.asarray(item[0], dtype=np.uint16)
                if batch and (len(batch) == _LEARN_BATCH or batch[0][0].shape != depth.shape):
                    flush()
                batch.append((depth, np.asarray(item[1]), item[2], item[3], item[4]))
            flush()
            forest = tr.fit()
            self.last_stats = tr.stats()
        return forest, ModelParams(self.stepwidth, self.subimg_width, self.subimg_height, float(gaussian_sigma), 20)

    def learn_biwi(self, gaussian_sigma: float, reader, persons) -> tuple[Forest, ModelParams]:
        """Train on the given persons of a `biwi.BiwiReader` (masks are PNG files: decoded with Pillow)."""
        try:
            from PIL import Image
        except ImportError as e:   # pragma: no cover - depends on the environment
            raise RuntimeError("learn_biwi needs Pillow to decode the BIWI mask PNGs (pip install pillow)") from e

        def frames():
            for nr in persons:
                for dt in reader.person(nr):
                    mask = np.asarray(Image.open(dt.mask_path).convert("L"))
                    yield dt.depth, mask, dt.intrinsic, dt.trans.pos3d, dt.trans.rot

        return self.learn(gaussian_sigma, frames())

    def to_json(self) -> str:
        """The serde shape of `HoughLearning` (the `_param.json` of examples/hough_tree_trainer.rs)."""
        w, h = self.subimg_width, self.subimg_height
        tree = {"input_size": {"topleft": [0, 0], "bottomright": [w, h]},
                "min_subrect_factor": self.subrect_feature_scale, "max_subrect_factor": self.subrect_feature_scale,
                "number_of_gen_features": self.feature_number_per_node, "steepness": self.steepness_weighting,
                "max_depth": self.max_depth, "min_subset_size": self.min_subset_size_to_stop}   # (phantom: skip_serializing)
        return json.dumps({"stepwidth": self.stepwidth,
                           "learn_params": {"tree_param": tree, "number_of_trees": self.num_of_trees,
                                            "size_of_subset_per_training": self.subset_size_per_tree}})


def synthetic_truth(w: int, h: int, seed: int):
    """Training truth for `synth.biwi_like(w, h, seed)`: (depth, mask, K, pos3d, rot_deg).  The mask is the head's
    silhouette (holes included, as BIWI masks are), pos3d the sphere centre in camera space (mm), rot_deg the
    frame's `synth.head_truth` rotation."""
    from . import synth
    z0, hx, hy, rot = synth.head_truth(w, h, seed)
    depth = synth.biwi_like(w, h, seed)
    K = synth.default_intrinsic(w, h)
    fx = float(K[0, 0])
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    dxm, dym = (xx - hx) * z0 / fx, (yy - hy) * z0 / fx
    mask = (dxm * dxm + dym * dym < 95.0 * 95.0).astype(np.uint8)
    pos3d = np.array([(hx - K[0, 2]) * z0 / fx, (hy - K[1, 2]) * z0 / float(K[1, 1]), z0], dtype=np.float32)
    return depth, mask, K, pos3d, np.asarray(rot, dtype=np.float32)


def synthetic_data(n: int, w: int = 320, h: int = 240, first: int = 0):
    """`n` frames of `synthetic_truth` from the canonical stream (seed = synth.FRAME_SEED_BASE + index)."""
    from . import synth
    for i in range(n):
        yield synthetic_truth(w, h, synth.FRAME_SEED_BASE + first + i)


# ------------------------------------------------------------------ rendered subjects: a head whose rotation can be observed
RENDER_SEED_BASE = 0x4EAD0000
RENDER_BATCH = 64
YAW, PITCH, ROLL = 1, 2, 0    # index of each angle in rot_deg: the viewer turns about y by rot[1], about x by rot[2], about z by rot[0]


def rendered_pose(w: int, h: int, seed: int, yaw=(-40, 40), pitch=(-20, 20), roll=(-10, 10)):
    """(pos3d [3] f32 mm, rot_deg [3] f32) of rendered frame `seed`: the head centre where `synth.head_truth` puts its sphere
    (700 - 1200 mm, the middle half of the frame), the angles uniform in their ranges (degrees)."""
    from . import synth
    u = synth.SplitMix(seed).uniform(6)
    K = synth.default_intrinsic(w, h)
    z0 = 700.0 + 500.0 * u[0]
    hx, hy = w * (0.25 + 0.5 * u[1]), h * (0.25 + 0.5 * u[2])
    pos3d = np.array([(hx - K[0, 2]) * z0 / K[0, 0], (hy - K[1, 2]) * z0 / K[1, 1], z0], dtype=np.float32)
    rot = np.zeros(3, dtype=np.float32)
    for axis, rng, ui in ((YAW, yaw, u[3]), (PITCH, pitch, u[4]), (ROLL, roll, u[5])):
        rot[axis] = rng[0] + (rng[1] - rng[0]) * ui
    return pos3d, rot


def rendered_data(n: int, w: int = 320, h: int = 240, first: int = 0, mesh=None, yaw=(-40, 40), pitch=(-20, 20), roll=(-10, 10),
                  device: int = 0, noise: int = 2, holes: float = 0.02):
    """`n` frames of a head mesh rendered on the GPU, as the (depth, mask, K, pos3d, rot_deg) tuples `synthetic_data` yields:
    frame i (seed RENDER_SEED_BASE + first + i) holds the head (`mesh`: (verts, tris), default `synth.head_mesh()`) at
    `rendered_pose`, turned by `render.euler_to_matrix(rot_deg)`, and a torso box that is not a head below it, its front 50 mm
    behind the head centre; +-`noise` mm and `holes` as `synth.biwi_like`.  Rendered RENDER_BATCH frames at a time."""
    from . import render, synth
    verts, tris = synth.head_mesh() if mesh is None else mesh
    K = synth.default_intrinsic(w, h)
    with render.Mesh(verts, tris, device) as head, render.Mesh(*synth.box_mesh((-142.0, 85.0, 50.0), (142.0, 700.0, 250.0)), device) as torso, \
            render.Renderer(device) as rd:
        for b0 in range(0, n, RENDER_BATCH):
            nb = min(RENDER_BATCH, n - b0)
            poses = [rendered_pose(w, h, RENDER_SEED_BASE + first + b0 + i, yaw, pitch, roll) for i in range(nb)]
            items = []
            for i, (pos, rot) in enumerate(poses):
                items.append((i, 0, render.euler_to_matrix(rot), pos, 1.0, True))
                items.append((i, 1, np.eye(3, dtype=np.float32), pos, 1.0, False))
            frames, masks = rd.render([head, torso], render.instances(items), nb, w, h, K, noise=noise, holes=holes,
                                      seed=RENDER_SEED_BASE + first + b0)
            for i, (pos, rot) in enumerate(poses):
                yield frames[i], masks[i], K, pos, rot

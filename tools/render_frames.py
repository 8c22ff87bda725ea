"""Render a batch of posed heads to files: `frames.npy` (u16 [n, h, w]), `masks.npy` (u8), `poses.npy` (pos3d and rot_deg per
frame) and `K.npy` in `--out`, and with `--bin` every frame also as a BIWI-style run-length `frame_%05d_depth.bin`
(`biwi.encode_depth`), for people who want files rather than device buffers."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--bin", action="store_true", help="also write BIWI run-length .bin depth files")
    ap.add_argument("--obj", help="a Wavefront OBJ head mesh (mm, camera frame) in place of synth.head_mesh()")
    a = ap.parse_args()
    from depthhead_amd import biwi, render, training
    w, h = (int(v) for v in a.size.split("x"))
    mesh = None
    if a.obj:
        with open(a.obj) as f:
            mesh = render.parse_obj(f.read())
    data = list(training.rendered_data(a.frames, w, h, first=a.first, mesh=mesh))
    os.makedirs(a.out, exist_ok=True)
    np.save(os.path.join(a.out, "frames.npy"), np.stack([d[0] for d in data]))
    np.save(os.path.join(a.out, "masks.npy"), np.stack([d[1] for d in data]))
    np.save(os.path.join(a.out, "poses.npy"), np.stack([np.concatenate([d[3], d[4]]) for d in data]))
    np.save(os.path.join(a.out, "K.npy"), data[0][2])
    if a.bin:
        for i, d in enumerate(data):
            with open(os.path.join(a.out, "frame_%05d_depth.bin" % (a.first + i)), "wb") as f:
                f.write(biwi.encode_depth(d[0]))
    print(f"{a.frames} frames of {w}x{h} -> {a.out}")


if __name__ == "__main__":
    main()

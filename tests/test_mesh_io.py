"""The OBJ reader on a hand-written file, and the procedural head of synth.head_mesh: closed, and not the same from the front
as from the back (nor from above as from below), which is what makes its rotation observable."""
from collections import Counter

import numpy as np
import pytest

from depthhead_amd import render, synth

OBJ = """# a unit cube: quads, a pentagon split by hand into a quad and a triangle, negative indices, v/vt/vn faces
o cube
v 0 0 0
v 1 0 0   # trailing comment
v 1 1 0
v 0 1 0
vt 0.5 0.5
vn 0 0 1
f 1 4 3 2
v 0 0 1
v 1 0 1
v 1 1 1
v 0 1 1
f 5/1/1 6/1/1 7/1/1 8/1/1
f -8 -7 -3 -4
f 2//1 3//1 7//1 6//1
s off
f -6/1 -5/1 -1/1 -2/1
usemtl none
f 4 1 5
f 4 5 8
"""


def test_obj_reader_quads_negative_indices_and_suffixes(tmp_path):
    v, t = render.parse_obj(OBJ)
    assert v.dtype == np.float32 and t.dtype == np.uint32 and v.shape == (8, 3) and t.shape == (12, 3)
    assert np.array_equal(v[6], [1, 1, 1]) and np.array_equal(v[1], [1, 0, 0])
    assert t[0].tolist() == [0, 3, 2] and t[1].tolist() == [0, 2, 1]                 # the fan of f 1 4 3 2
    assert t[2].tolist() == [4, 5, 6] and t[3].tolist() == [4, 6, 7]                 # v/vt/vn
    assert t[4].tolist() == [0, 1, 5] and t[5].tolist() == [0, 5, 4]                 # -8 -7 -3 -4 with eight vertices read
    assert t[6].tolist() == [1, 2, 6] and t[8].tolist() == [2, 3, 7]                 # v//vn, and -6 -5 -1 -2
    edges = Counter(tuple(sorted((int(a), int(b)))) for tri in t for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])))
    assert set(edges.values()) == {2}                                                # the cube is closed
    # negative indices count back from the vertices read SO FAR
    v2, t2 = render.parse_obj("v 0 0 0\nv 1 0 0\nv 0 1 0\nf -3 -2 -1\nv 5 5 5\nf -1 -2 -3\n")
    assert t2.tolist() == [[0, 1, 2], [3, 2, 1]]
    for bad in ("v 0 0 0\nf 1 2 3\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf -4 1 2\n", "v 1 2\n", "v 0 0 0\nv 1 1 1\nf 1 2\n"):
        with pytest.raises(ValueError):
            render.parse_obj(bad)
    p = tmp_path / "cube.obj"
    p.write_text(OBJ)
    assert callable(render.Mesh.from_obj)
    with open(p) as f:
        assert np.array_equal(render.parse_obj(f.read())[1], t)


@pytest.mark.parametrize("subdiv", [0, 2, 3])
def test_head_mesh_is_closed(subdiv):
    v, t = synth.head_mesh(subdiv)
    assert v.dtype == np.float32 and t.dtype == np.uint32
    assert len(t) == 20 * 4 ** subdiv and len(v) == 10 * 4 ** subdiv + 2 and t.max() == len(v) - 1
    edges = Counter(tuple(sorted((int(a), int(b)))) for tri in t for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])))
    assert set(edges.values()) == {2}                                                # every edge is shared by exactly two triangles
    directed = Counter((int(a), int(b)) for tri in t for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])))
    assert set(directed.values()) == {1}                                             # and consistently wound
    assert np.isfinite(v).all() and len(np.unique(v, axis=0)) == len(v)


def test_head_mesh_is_a_head_not_a_sphere():
    v, _ = synth.head_mesh()
    assert len(v) == 642
    lo, hi = v.min(axis=0), v.max(axis=0)
    assert 74 <= hi[0] <= 76 and 74 <= -lo[0] <= 76                                  # 75 mm half width
    assert 104 <= -lo[1] <= 106 and 104 <= hi[1] <= 112                              # 105 mm up, the chin a little further down
    assert 94 <= hi[2] <= 96 and 115 <= -lo[2] <= 125                                # 95 mm back, the nose about 120 mm to the front
    # not mirror-symmetric front to back: flipping z moves the vertex set (Hausdorff distance of the two sets, one way)
    def one_way(a, b):
        return max(np.sqrt(((b - p) ** 2).sum(axis=1)).min() for p in a)
    assert one_way(v, v * np.float32([1, 1, -1])) > 15.0
    assert one_way(v, v * np.float32([1, -1, 1])) > 5.0                              # nor top to bottom: pitch is observable
    assert one_way(v, v * np.float32([-1, 1, 1])) < 1e-3                             # left and right are alike
    nose = v[np.argmin(v[:, 2])]
    assert abs(nose[0]) < 1.0 and 0 < nose[1] < 30                                   # the nose: in the middle, a little below the centre


def test_euler_to_matrix_is_the_convention_of_world_rotation():
    from depthhead_amd.tracking import world_rotation
    for rot in ((0, 0, 0), (10, -25, 7), (-170, 80, 33), (0, 90, 0)):
        m = render.euler_to_matrix(rot)
        assert m.dtype == np.float32 and m.shape == (3, 3)
        assert np.abs(m - world_rotation(np.eye(3), np.radians(np.float64(rot)))).max() < 1e-7
    # yaw (rot[1]) turns the nose direction (0, 0, -1) sideways, pitch (rot[2]) up or down
    assert np.allclose(render.euler_to_matrix((0, 90, 0)) @ [0, 0, -1], [-1, 0, 0], atol=1e-6)
    assert np.allclose(render.euler_to_matrix((0, 0, 90)) @ [0, 0, -1], [0, 1, 0], atol=1e-6)

"""The rendering rule of DESIGN.md section 17 (include/depthhead_hip.h, "rendering posed meshes") restated in numpy, one triangle
at a time: f32 vertex arithmetic with every product and sum rounded on its own, int64 edge functions with the top-left rule,
f64 depth in the stated order, a minimum over keys.  Written from the section, not from the kernels; test_gpu_render.py holds
the GPU to it bit for bit and test_render_ref.py holds it to cases with answers known on paper."""
import numpy as np

F32 = np.float32
GUARD = 1 << 20
EMPTY = np.uint32(0xFFFFFFFF)
HEAD = 1


def instance(frame, mesh, R=None, t=(0, 0, 0), scale=1.0, head=True):
    """One instance as a plain dict (the fields of dh_render_instance)."""
    R = np.eye(3) if R is None else R
    return {"frame": int(frame), "mesh": int(mesh), "R": np.asarray(R, dtype=F32).reshape(3, 3), "t": np.asarray(t, dtype=F32).reshape(3),
            "scale": F32(scale), "flags": HEAD if head else 0}


def transform(verts, R, t, scale):
    """p[j] = ((R[j][0] * sv0 + R[j][1] * sv1) + R[j][2] * sv2) + t[j], sv = v * scale, in f32."""
    v = np.asarray(verts, dtype=F32).reshape(-1, 3)
    sv = v * F32(scale)
    p = np.empty_like(sv)
    for j in range(3):
        p[:, j] = ((R[j, 0] * sv[:, 0] + R[j, 1] * sv[:, 1]) + R[j, 2] * sv[:, 2]) + t[j]
    return p


def project(K, p):
    """to2d: r = K p in the reference's mat-vec order (t = p0 * m[j][0]; t += p1 * m[j][1]; t += p2 * m[j][2]), x = r0 / r2,
    y = r1 / r2; then the snap s = floorf(x * 16 + 0.5), kept in f32."""
    K = np.asarray(K, dtype=F32).reshape(3, 3)
    with np.errstate(all="ignore"):
        r = [(p[:, 0] * K[j, 0] + p[:, 1] * K[j, 1]) + p[:, 2] * K[j, 2] for j in range(3)]
        x, y = r[0] / r[2], r[1] / r[2]
        return np.floor(x * F32(16.0) + F32(0.5)), np.floor(y * F32(16.0) + F32(0.5))


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def _owns(ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    return dy < 0 or (dy == 0 and dx > 0)


def draw_triangle(keys, sx, sy, pz, low):
    """One triangle (snapped int coordinates, f32 depths of its three vertices) into the u32 key image of its frame."""
    h, w = keys.shape
    x, y, z = [int(v) for v in sx], [int(v) for v in sy], [F32(v) for v in pz]
    area = _edge(x[0], y[0], x[1], y[1], x[2], y[2])
    if area == 0:
        return
    if area < 0:                                       # both windings are drawn: vertices 1 and 2 change places
        x[1], x[2], y[1], y[2], z[1], z[2] = x[2], x[1], y[2], y[1], z[2], z[1]
    # pixels whose centre 16 x + 8 lies in the bounding box
    xa, xb = max(-((8 - min(x)) // 16), 0), min((max(x) - 8) // 16, w - 1)
    ya, yb = max(-((8 - min(y)) // 16), 0), min((max(y) - 8) // 16, h - 1)
    if xa > xb or ya > yb:
        return
    py, px = np.meshgrid(np.arange(ya, yb + 1, dtype=np.int64) * 16 + 8, np.arange(xa, xb + 1, dtype=np.int64) * 16 + 8, indexing="ij")
    e = [_edge(x[1], y[1], x[2], y[2], px, py), _edge(x[2], y[2], x[0], y[0], px, py), _edge(x[0], y[0], x[1], y[1], px, py)]
    own = [_owns(x[1], y[1], x[2], y[2]), _owns(x[2], y[2], x[0], y[0]), _owns(x[0], y[0], x[1], y[1])]
    inside = np.ones(px.shape, dtype=bool)
    for ei, oi in zip(e, own):
        inside &= (ei >= 0) if oi else (ei > 0)
    if not inside.any():
        return
    iz = [np.float64(1.0) / np.float64(zi) for zi in z]
    e0, e1, e2 = (ei[inside] for ei in e)
    with np.errstate(all="ignore"):
        zz = (e0 + e1 + e2).astype(np.float64) / ((e0.astype(np.float64) * iz[0] + e1.astype(np.float64) * iz[1]) + e2.astype(np.float64) * iz[2])
        zz = zz + 0.5
        d = np.where(zz >= 1.0, np.where(zz >= 65535.0, 65535.0, np.floor(zz)), 1.0).astype(np.uint32)     # (NaN -> 1)
    key = (d << np.uint32(1)) | np.uint32(low)
    sub = keys[ya:yb + 1, xa:xb + 1]
    sub[inside] = np.minimum(sub[inside], key)


def render_keys(meshes, instances, n, w, h, K):
    """The resolved key image [n, h, w] u32 (EMPTY where nothing was drawn).  meshes: list of (verts [nv, 3], tris [nt, 3]);
    K: one 3 x 3 or [n, 3, 3]."""
    K = np.asarray(K, dtype=F32)
    Ks = np.broadcast_to(K.reshape(-1, 3, 3), (n, 3, 3)) if K.size == 9 else K.reshape(n, 3, 3)
    keys = np.full((n, h, w), EMPTY, dtype=np.uint32)
    for ins in instances:
        verts, tris = meshes[ins["mesh"]]
        tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
        p = transform(verts, ins["R"], ins["t"], ins["scale"])
        fx, fy = project(Ks[ins["frame"]], p)
        with np.errstate(invalid="ignore"):
            ok = ~(p[:, 2] < F32(1.0)) & (np.abs(fx) <= F32(GUARD)) & (np.abs(fy) <= F32(GUARD))      # (NaN and infinity fail)
        sx, sy = np.where(ok, fx, 0).astype(np.int64), np.where(ok, fy, 0).astype(np.int64)
        low = 0 if ins["flags"] & HEAD else 1
        for tri in tris:
            if ok[tri].all():
                draw_triangle(keys[ins["frame"]], sx[tri], sy[tri], p[tri, 2], low)
    return keys


_G, _M1, _M2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def splitmix_at(seed, c):
    """Output number c (from 0) of the splitmix64 stream seeded with `seed` (what synth.SplitMix(seed).u64 yields)."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + (np.asarray(c, dtype=np.uint64) + np.uint64(1)) * _G
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def resolve(keys, noise=0, holes=0.0, seed=0):
    """(frames u16, masks u8) of a key image, with the sensor model."""
    fg = keys != EMPTY
    d = np.where(fg, keys >> np.uint32(1), 0).astype(np.int64)
    mask = (fg & ((keys & np.uint32(1)) == 0)).astype(np.uint8)
    if noise or holes:
        k = np.arange(keys.size, dtype=np.uint64).reshape(keys.shape)
        u0, u1 = splitmix_at(seed, np.uint64(2) * k), splitmix_at(seed, np.uint64(2) * k + np.uint64(1))
        nz = (u0 % np.uint64(2 * noise + 1)).astype(np.int64) - noise
        thr = np.uint64(int(np.floor(holes * 9007199254740992.0)))
        d = np.where(fg, np.clip(d + nz, 1, 65535), 0)
        d = np.where(fg & ((u1 >> np.uint64(11)) < thr), 0, d)
    return d.astype(np.uint16), mask


def render(meshes, instances, n, w, h, K, noise=0, holes=0.0, seed=0):
    return resolve(render_keys(meshes, instances, n, w, h, K), noise, holes, seed)

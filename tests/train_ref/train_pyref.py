"""Second restatement of the trainer contract in plain Python (scalar loops, numpy.float32 for the f32 steps), for tiny
configurations only: tests/test_train_cpu.py holds the C oracle to it bit for bit."""
from __future__ import annotations

import math

import numpy as np

M64 = 0xFFFFFFFFFFFFFFFF
G = 0x9E3779B97F4A7C15


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key(seed, tag, a, b):
    h = mix64((seed + (tag + 1) * G) & M64)
    h = mix64((h + (a + 1) * G) & M64)
    return mix64((h + (b + 1) * G) & M64)


def u01(u):
    return (u >> 11) * (1.0 / 9007199254740992.0)


def inv3(m):
    f = np.float32
    a, b, c, d, e, ff, g, h, i = (f(x) for x in m)
    det = a * (e * i - ff * h) - d * (b * i - c * h) + g * (b * ff - c * e)
    return [(e * i - ff * h) / det, (c * h - b * i) / det, (b * ff - c * e) / det, (ff * g - d * i) / det, (a * i - c * g) / det,
            (c * d - a * ff) / det, (d * h - e * g) / det, (b * g - a * h) / det, (a * e - b * d) / det]


class Trainer:
    def __init__(self, p):
        self.p = p
        self.frames = 0
        self.patches, self.lab, self.off, self.rot = [], [], [], []
        self.where = []   # (frame index over every frame added, x, y) of each sample's window centre

    def add(self, frames, masks, K, pos3d, rot_deg):
        p = self.p
        W, H, st = p.subimage_width, p.subimage_height, p.stepwidth
        lw, lh = W // 2, H // 2
        n, h, w = frames.shape
        for f in range(n):
            img, mask = frames[f].astype(np.int64), masks[f]
            xs = list(range(lw, w - (W - lw), st))
            ys = list(range(lh, h - (H - lh), st))
            cls = ([], [])
            for iy, y in enumerate(ys):
                for ix, x in enumerate(xs):
                    if not int(img[y - lh:y - lh + H, x - lw:x - lw + W].sum()) > 0:
                        continue
                    i = iy * len(xs) + ix
                    cls[1 if mask[y, x] else 0].append((key(p.seed, 1, self.frames + f, i), i))
            kinv = inv3(K[f])
            for c in (0, 1):
                for _, i in sorted(cls[c])[:20]:
                    x, y = xs[i % len(xs)], ys[i // len(xs)]
                    off, rot = [np.float32(0)] * 3, [0.0] * 3
                    if c:
                        v = (np.float32(x), np.float32(y), np.float32(1))
                        r = []
                        for j in range(3):
                            t = v[0] * kinv[j * 3]
                            t = t + v[1] * kinv[j * 3 + 1]
                            t = t + v[2] * kinv[j * 3 + 2]
                            r.append(t)
                        cc = np.float32(frames[f][y, x]) / r[2]
                        off = [r[k] * cc - np.float32(pos3d[f][k]) for k in range(3)]
                        rot = [float(np.float32(rot_deg[f][k])) for k in range(3)]
                    self.patches.append(frames[f][y - lh:y - lh + H, x - lw:x - lw + W].astype(np.int64))
                    self.lab.append(c)
                    self.off.append([float(o) for o in off])
                    self.rot.append(rot)
                    self.where.append((self.frames + f, x, y))
        self.frames += n

    def fit(self):
        """-> (roots, nodes [(r1, r2, th, cz, co)], leaves [(prob, [offsets], [rotations])]) in breadth-first order."""
        p = self.p
        W, H, s = p.subimage_width, p.subimage_height, p.subrect_feature_scale
        rw, rh = int(W * s), int(H * s)
        pool = len(self.lab)

        def avg(smp, x, y):
            if rw * rh == 0:
                return 0.0
            return float(int(self.patches[smp][y:y + rh, x:x + rw].sum())) / float(rw * rh)

        def cand(t, heap, c):
            a = (t << 32) | heap
            us = [u01(key(p.seed, 3, a, c * 8 + k)) for k in range(5)]
            cx = lambda L, u: int(0.0 + u * (float(L) - float(L) * s))  # noqa: E731
            return cx(W, us[0]), cx(H, us[1]), cx(W, us[2]), cx(H, us[3]), -256.0 + us[4] * 512.0

        def side(k, smp):
            return 1 if avg(smp, k[0], k[1]) - avg(smp, k[2], k[3]) > k[4] else 0

        ln0 = lambda x: 0.0 if x == 0.0 else math.log(x)  # noqa: E731

        def entropy(st):
            pr = sum(self.lab[i] for i in st) / len(st)
            return pr * ln0(pr) + (1.0 - pr) * ln0(1.0 - pr)

        def det(m):
            return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[1][0] * (m[0][1] * m[2][2] - m[0][2] * m[2][1])
                    + m[2][0] * (m[0][1] * m[1][2] - m[0][2] * m[1][1]))

        def cov(vs):
            mean = list(vs[0])
            for v in vs[1:]:
                mean = [mean[k] + v[k] for k in range(3)]
            mean = [m / len(vs) for m in mean]
            c = None
            for v in vs:
                d = [v[k] - mean[k] for k in range(3)]
                o = [[d[a] * d[b] for b in range(3)] for a in range(3)]
                c = o if c is None else [[c[a][b] + o[a][b] for b in range(3)] for a in range(3)]
            with np.errstate(invalid="ignore"):
                return [[float(np.float64(c[a][b]) / np.float64(len(vs) - 1)) for b in range(3)] for a in range(3)]

        def reg(st):
            pos = [i for i in st if self.lab[i]]
            if not pos:
                return 0.0
            x = det(cov([self.off[i] for i in pos])) + det(cov([self.rot[i] for i in pos]))
            return math.log(x) if x > 0.0 else 0.0

        def impurity(l, r, depth):
            n = len(l) + len(r)
            lf, rf = len(l) / n, len(r) / n
            return -(lf * entropy(l) + rf * entropy(r)) + (1.0 - math.exp(-(depth / p.steepness))) * (lf * reg(l) + rf * reg(r))

        roots, nodes, leaves = [], [], []
        for t in range(p.n_trees):
            root = [(key(p.seed, 2, t, i) * pool) >> 64 for i in range(p.subset_per_tree)]
            queue = [(1, -1, 0, root)]
            while queue:
                heap, parent, sd, st = queue.pop(0)
                depth = heap.bit_length() - 1
                best, bs = None, None
                if any(self.lab[i] for i in st) and depth < p.max_depth and len(st) >= p.min_subset_size:
                    for c in range(p.features_per_node):
                        k = cand(t, heap, c)
                        l = [i for i in st if not side(k, i)]
                        r = [i for i in st if side(k, i)]
                        if l and r:
                            sc = impurity(l, r, depth)
                            if bs is None or sc < bs:
                                best, bs = k, sc
                if best is None:
                    ref = ~len(leaves)
                    pos = [i for i in st if self.lab[i]]
                    leaves.append((len(pos) / len(st) if st else 0.0, [self.off[i] for i in pos], [self.rot[i] for i in pos]))
                else:
                    ref = len(nodes)
                    nodes.append([(best[0], best[1], best[0] + rw, best[1] + rh), (best[2], best[3], best[2] + rw, best[3] + rh),
                                  best[4], 0, 0])
                    queue.append((2 * heap, ref, 0, [i for i in st if not side(best, i)]))
                    queue.append((2 * heap + 1, ref, 1, [i for i in st if side(best, i)]))
                if parent < 0:
                    roots.append(ref)
                else:
                    nodes[parent][3 + sd] = ref
        return roots, nodes, leaves

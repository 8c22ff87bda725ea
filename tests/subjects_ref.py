"""A shape per subject (include/depthhead_hip.h, "a shape per subject") restated in numpy: the update of a
subject set -- apply, points from the base, normals as a gather over each vertex's corner list, one square root -- the shape step
over a set and the driver.  f64 with every operation rounded on its own; the shape step's sums are shape_ref's Python ints and
the fit is fit_ref's.  Written from the header text, not from the kernels.  test_subjects_ref.py holds it to fit.deform and
fit.vertex_normals byte for byte and to shape_ref.adapt; test_gpu_subjects.py holds the GPU to it with no tolerance."""
import numpy as np

import fit_ref as fr
import shape_ref as sr
from fit_ref import F64

CLAMPED, NONFINITE = 1, 2
# dh_subject_state, 80 bytes without padding
STATE_DTYPE = np.dtype([("coeffs", "<f8", (8,)), ("applied", "<u4"), ("rejected", "<u4"), ("flags", "<u4"), ("zero_normals", "<u4")])
assert STATE_DTYPE.itemsize == 80
U32_MAX = 0xFFFFFFFF


def corner_lists(tris, n):
    """(begin [n + 1], corners [3 m]) as Python-int arrays: vertex v's incident corners, corner t * 3 + c being corner c of
    triangle t, in ascending order."""
    flat = [int(v) for v in np.asarray(tris).reshape(-1)]
    runs = [[] for _ in range(n)]
    for q, v in enumerate(flat):
        runs[v].append(q)
    begin = [0]
    for r in runs:
        begin.append(begin[-1] + len(r))
    return np.array(begin, np.int64), np.array([q for r in runs for q in r], np.int64)


def radius_bound(verts, basis, max_coeff):
    """radius(base) + (K * max_coeff) * largest |B_k[i]|, each as the library computes it."""
    def largest(x):
        x = np.asarray(x, np.float32).astype(F64).reshape(-1, 3)
        return np.sqrt(((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]).max())
    return F64(largest(verts)) + (F64(len(basis)) * F64(max_coeff)) * F64(largest(basis))


def points(verts, basis, coeffs):
    """POINTS: from the base, x = x + c_k * B_k for k ascending in f64, rounded to f32 once."""
    x = np.asarray(verts, dtype=np.float32).astype(F64).reshape(-1, 3)
    B = np.asarray(basis, dtype=np.float32).astype(F64)
    for k in range(len(B)):
        x = x + F64(coeffs[k]) * B[k]
    return x.astype(np.float32)


def normals(pts, tris, lists=None):
    """NORMALS of the f32 points: (normals [n, 3] f32, the count of vertices whose normal is zero).  The face products per
    triangle, then per vertex m = +0.0 and m = m + f over its corner list in list order (all vertices at once, one list
    position after the other), q, the square root and the division."""
    v = np.asarray(pts, dtype=np.float32).astype(F64).reshape(-1, 3)
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    begin, corners = lists if lists is not None else corner_lists(t, len(v))
    with np.errstate(all="ignore"):
        u, w = v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]
        f = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)
        m = np.zeros_like(v)
        degree = begin[1:] - begin[:-1]
        for r in range(int(degree.max()) if len(degree) else 0):
            has = np.flatnonzero(degree > r)
            m[has] = m[has] + f[corners[begin[has] + r] // 3]
        q = (m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]
        ln = np.sqrt(q)
        zero = ~(ln > 0.0)
        out = (m / np.where(zero, 1.0, ln)[:, None]).astype(np.float32)
    return out, int(zero.sum())


def apply(state, rec, nk, max_coeff):
    """APPLY of one subject: the state after its shape record."""
    st = state.copy()
    if int(rec["status"]) != sr.OK:
        return st
    delta = np.asarray(rec["delta"], F64)[:nk]
    if not np.isfinite(delta).all():
        st["rejected"] = min(int(st["rejected"]) + 1, U32_MAX)
        st["flags"] = int(st["flags"]) | NONFINITE
        return st
    hi = F64(max_coeff)
    for k in range(nk):
        with np.errstate(all="ignore"):
            c = F64(st["coeffs"][k]) + delta[k]
        if c > hi:
            c = hi
            st["flags"] = int(st["flags"]) | CLAMPED
        if c < -hi:
            c = -hi
            st["flags"] = int(st["flags"]) | CLAMPED
        st["coeffs"][k] = c
    st["applied"] = min(int(st["applied"]) + 1, U32_MAX)
    return st


class Set:
    """The restated dh_fit_subjects: state [S], pts and nrm [S, n, 3] f32."""

    def __init__(self, verts, tris, basis, n_subjects, max_coeff=0.5):
        self.verts = np.asarray(verts, np.float32).reshape(-1, 3)
        self.tris = np.asarray(tris, np.int64).reshape(-1, 3)
        self.basis = np.asarray(basis, np.float32)
        self.nk, self.max_coeff = len(self.basis), float(max_coeff)
        self.lists = corner_lists(self.tris, len(self.verts))
        self.radius = radius_bound(self.verts, self.basis, max_coeff)
        self.state = np.zeros(n_subjects, STATE_DTYPE)
        self.pts = np.zeros((n_subjects, len(self.verts), 3), np.float32)
        self.nrm = np.zeros_like(self.pts)
        self.evaluate(range(n_subjects))

    def __len__(self):
        return len(self.state)

    def evaluate(self, which):
        for s in which:
            self.pts[s] = points(self.verts, self.basis, self.state["coeffs"][s])
            self.nrm[s], self.state["zero_normals"][s] = normals(self.pts[s], self.tris, self.lists)

    def set_coeffs(self, coeffs, first=0):
        c = np.asarray(coeffs, F64)
        c = c.reshape(-1, c.shape[-1])
        for i in range(len(c)):
            self.state["coeffs"][first + i] = 0.0
            self.state["coeffs"][first + i, :self.nk] = c[i, :self.nk]
            self.state["flags"][first + i] = 0
        self.evaluate(range(first, first + len(c)))

    def update(self, records):
        for s in range(len(self.state)):
            self.state[s] = apply(self.state[s], records[s], self.nk, self.max_coeff)
        self.evaluate(range(len(self.state)))


def shape_step(frames, Ks, st, instances, subjects=None, n_subjects=None, fit_status=None, prm=None):
    """THE SHAPE STEP OVER A SET: sr.RECORD_DTYPE [n_subjects], every instance at its own subject's model; an instance whose
    fit_status is not OK takes no part."""
    prm = prm or sr.params()
    n_subjects = len(st) if n_subjects is None else n_subjects
    Ks = np.asarray(Ks, dtype=np.float32)
    nk = st.nk
    sums = [[{(k, l): 0 for k in range(nk) for l in range(k, nk)}, [0] * nk, 0, 0, 0] for _ in range(n_subjects)]
    for i, inst in enumerate(instances):
        sj = 0 if subjects is None else int(subjects[i])
        if sj == sr.SKIP or (fit_status is not None and int(fit_status[i]) != fr.OK):
            continue
        f = int(inst["frame"])
        A, b, e, count = sr.instance_sums(frames[f], Ks if Ks.ndim == 2 else Ks[f], st.pts[sj], st.nrm[sj], st.basis, inst, prm["gate"])
        s = sums[sj]
        for key, v in A.items():
            s[0][key] += v
        s[1] = [p + q for p, q in zip(s[1], b)]
        s[2] += e
        s[3] += count
        s[4] += 1 if count > 0 else 0
    out = np.zeros(n_subjects, sr.RECORD_DTYPE)
    for sj, (A, b, e, count, used) in enumerate(sums):
        out[sj] = sr.solve_subject(A, b, e, count, used, nk, prm)
    return out


def adapt_subjects(frames, K, st, starts, subject_of, rounds=6, fit_prm=None, shape_prm=None):
    """fit.adapt_subjects restated: `starts` a list of instance dicts (frame, R, t, scale).  Returns (the set's state, the last
    instances, (the last round's fit records, its shape records), trace of (coefficients [S, 8], fit records, shape records))."""
    inst = [dict(s) for s in starts]
    recs = srec = None
    trace = []
    for _ in range(rounds):
        recs = []
        for s, sj in zip(inst, subject_of):
            R, t, rec = fr.fit(frames[s["frame"]], K, st.pts[sj], st.nrm[sj], s["R"], s["t"], s["scale"], fit_prm)
            s["R"], s["t"] = R, t
            recs.append(rec)
        srec = shape_step(frames, K, st, inst, subject_of, len(st), [r["status"] for r in recs], shape_prm)
        trace.append((st.state["coeffs"].copy(), recs, srec))
        st.update(srec)
    return st.state.copy(), inst, (recs, srec), trace

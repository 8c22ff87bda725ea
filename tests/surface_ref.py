"""A surface per subject (include/depthhead_hip.h, "a surface per subject") restated in numpy: the neighbour
lists, the grown radius bound, the points of a surface set, the surface step -- accumulate into int64 words per vertex, the Jacobi
solve, the finite test and the clamp, the record -- and the driver.  f64 with every operation rounded on its own; the sums are
int64 and Python ints.  Written from the header text, not from the kernels: the point's p, nrm, c, pixel, d and residual are the
fit's one pass, so those lines follow fit_ref.one_pass expression for expression.  test_surface_ref.py holds it to scenes whose
answer is known; test_gpu_surface.py holds the GPU to it with no tolerance."""
import numpy as np

import fit_ref as fr
import shape_ref as sr
import subjects_ref as sb
from fit_ref import F64, S

OK, FEW_POINTS = 0, 1
MAX_OFFSET, MAX_SCALE, MAX_ITERATIONS, MAX_CELLS = 64.0, 64.0, 256, 1 << 22
NB_BOUND = 1.01
R_TOLERANCE, MAX_EXTENT, MAX_FIELD = 0.02, 4096.0, 256.0       # DH_FIT_R_TOLERANCE, DH_FIT_MAX_EXTENT, DH_SHAPE_MAX_FIELD
# dh_surface_record, 40 bytes without padding
RECORD_DTYPE = np.dtype([("status", "<u4"), ("points", "<u4"), ("instances", "<u4"), ("observed", "<u4"), ("clamped", "<u4"),
                         ("rejected", "<u4"), ("sum_r2_fixed", "<i8"), ("max_abs", "<f8")])
assert RECORD_DTYPE.itemsize == 40


def params(gate=25.0, min_cos2=0.25, mu=0.5, eps=0.05, min_count=2, min_points=64, iterations=32):
    return {"gate": float(gate), "min_cos2": float(min_cos2), "mu": float(mu), "eps": float(eps), "min_count": int(min_count),
            "min_points": int(min_points), "iterations": int(iterations)}


def neighbour_lists(tris, n):
    """(begin [n + 1], list): vertex v's neighbours -- the unique vertices other than v that share a triangle edge with it --
    ascending."""
    sets = [set() for _ in range(n)]
    for tri in np.asarray(tris, np.int64).reshape(-1, 3).tolist():
        for c in range(3):
            sets[tri[c]].update((tri[(c + 1) % 3], tri[(c + 2) % 3]))
    runs = [sorted(s - {v}) for v, s in enumerate(sets)]
    begin = [0]
    for r in runs:
        begin.append(begin[-1] + len(r))
    return np.array(begin, np.int64), np.array([j for r in runs for j in r], np.int64)


def radius_bound(verts, basis, max_coeff, max_offset):
    """Section 25's bound + max_offset * 1.01."""
    return sb.radius_bound(verts, basis, max_coeff) + F64(max_offset) * F64(NB_BOUND)


def points(verts, basis, coeffs, nb, offsets):
    """POINTS of a surface set: section 25's tree, then x = x + o_i * nb_i, rounded to f32 once."""
    x = np.asarray(verts, dtype=np.float32).astype(F64).reshape(-1, 3)
    B = np.asarray(basis, dtype=np.float32).astype(F64)
    for k in range(len(B)):
        x = x + F64(coeffs[k]) * B[k]
    x = x + np.asarray(offsets, F64)[:, None] * np.asarray(nb, np.float32).astype(F64)
    return x.astype(np.float32)


class Set(sb.Set):
    """The restated surface set: subjects_ref.Set with nb [n, 3] f32, the neighbour lists, offsets [S, n] f64 and the last step's
    counts [S, n]."""

    def __init__(self, verts, tris, basis, n_subjects, max_coeff=0.5, max_offset=16.0):
        v = np.asarray(verts, np.float32).reshape(-1, 3)
        B = np.asarray(basis, np.float32)
        self.max_offset = float(max_offset)
        self.nb = sb.normals(sb.points(v, B, np.zeros(len(B))), tris)[0]
        self.nbr = neighbour_lists(tris, len(v))
        self.offsets = np.zeros((n_subjects, len(v)), F64)
        self.counts = np.zeros((n_subjects, len(v)), np.int64)
        super().__init__(verts, tris, basis, n_subjects, max_coeff)
        self.radius = radius_bound(self.verts, self.basis, max_coeff, max_offset)
        b = self.basis.astype(F64).reshape(-1, 3)
        self.largest = np.sqrt(((b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2]).max())       # the basis's largest |B_k[i]|

    def evaluate(self, which):
        for s in which:
            self.pts[s] = points(self.verts, self.basis, self.state["coeffs"][s], self.nb, self.offsets[s])
            self.nrm[s], self.state["zero_normals"][s] = sb.normals(self.pts[s], self.tris, self.lists)

    def set_offsets(self, subject, offsets):
        o = np.asarray(offsets, F64).reshape(len(self.verts))
        assert (np.abs(o) <= self.max_offset).all()
        self.offsets[subject] = o
        self.evaluate([subject])


def instance_terms(frame, K, pts, nrm, nb, inst, prm):
    """(kept [n] bool, J [n], res [n]) of one instance: the fit's one pass at the instance's pose, the grazing test, and J along the
    base normal."""
    R = np.asarray(inst["R"], dtype=np.float32).reshape(3, 3).astype(F64)
    t = np.asarray(inst["t"], dtype=np.float32).reshape(3).astype(F64)
    scale = F64(np.float32(inst["scale"]))
    h, w = frame.shape
    K = np.asarray(K, dtype=np.float32).reshape(3, 3).astype(F64)
    v, m = np.asarray(pts, dtype=np.float32).astype(F64), np.asarray(nrm, dtype=np.float32).astype(F64)
    b = np.asarray(nb, dtype=np.float32).astype(F64)
    with np.errstate(all="ignore"):
        sv = v * scale
        p = [((R[j, 0] * sv[:, 0] + R[j, 1] * sv[:, 1]) + R[j, 2] * sv[:, 2]) + t[j] for j in range(3)]
        n = [(R[j, 0] * m[:, 0] + R[j, 1] * m[:, 1]) + R[j, 2] * m[:, 2] for j in range(3)]
        ok = p[2] >= 1.0
        c = (n[0] * p[0] + n[1] * p[1]) + n[2] * p[2]
        ok &= c < 0.0
        r = [(p[0] * K[j, 0] + p[1] * K[j, 1]) + p[2] * K[j, 2] for j in range(3)]
        x, y = r[0] / r[2], r[1] / r[2]
        ok &= (x >= 0.0) & (x < F64(w)) & (y >= 0.0) & (y < F64(h))
        px, py = np.where(ok, x, 0.0).astype(np.int64), np.where(ok, y, 0.0).astype(np.int64)
        d = frame[py, px].astype(F64)
        ok &= d != 0.0
        ok &= np.abs(d - p[2]) <= F64(prm["gate"])
        res = c * (d / p[2] - 1.0)
        ok &= c * c >= F64(prm["min_cos2"]) * ((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2])
        sbv = b * scale
        wv = [(R[j, 0] * sbv[:, 0] + R[j, 1] * sbv[:, 1]) + R[j, 2] * sbv[:, 2] for j in range(3)]
        J = (n[0] * wv[0] + n[1] * wv[1]) + n[2] * wv[2]
    return ok, J, res


def takes_part(inst, sj, n_subjects, n_frames, fit_status, radius, largest):
    """The step's per-instance rule as the device decides it (the host forms refuse what is not a skip): the subject and the fit
    record; the frame; then the per-instance refusals of sections 18 and 20 with the set's bound `radius` and the basis's
    `largest` -- R, t and scale finite, |R R^T - I| <= 0.02 per element, |scale| * radius <= 4096, |scale| * largest <= 256 -- and
    |scale| <= 64.  A NaN fails each test."""
    if sj == sr.SKIP or sj >= n_subjects or (fit_status is not None and int(fit_status) != fr.OK):
        return False
    if int(inst["frame"]) >= n_frames:
        return False
    R = np.asarray(inst["R"], dtype=np.float32).reshape(3, 3).astype(F64)
    t = np.asarray(inst["t"], dtype=np.float32).reshape(3).astype(F64)
    scale = F64(np.float32(inst["scale"]))
    if not (np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(scale)):
        return False
    for a in range(3):
        for b in range(a, 3):
            g = (R[a, 0] * R[b, 0] + R[a, 1] * R[b, 1]) + R[a, 2] * R[b, 2]
            if not abs(g - (1.0 if a == b else 0.0)) <= R_TOLERANCE:
                return False
    mag = abs(scale)
    return bool(mag * F64(radius) <= MAX_EXTENT and mag * F64(largest) <= MAX_FIELD and mag <= MAX_SCALE)


def solve(a, b, cnt, o, nbr, prm, max_offset):
    """SOLVE of one subject that has points enough: (offsets [n], observed, clamped, rejected)."""
    begin, lst = nbr
    deg = begin[1:] - begin[:-1]
    seen = cnt >= prm["min_count"]
    mu, eps = F64(prm["mu"]), F64(prm["eps"])
    with np.errstate(all="ignore"):
        A = np.where(seen, a.astype(F64) / S, 0.0)
        B = np.where(seen, b.astype(F64) / S, 0.0)
        c0 = A * o + B
        den = (A + mu * deg.astype(F64)) + eps
        u = o.copy()
        for _ in range(prm["iterations"]):
            s = np.zeros_like(u)
            for r in range(int(deg.max()) if len(deg) else 0):
                has = np.flatnonzero(deg > r)
                s[has] = s[has] + u[lst[begin[has] + r]]
            u = (c0 + mu * s) / den
        finite = (u - u) == 0.0
    u = np.where(finite, u, o)
    hi = F64(max_offset)
    over, under = finite & (u > hi), finite & (u < -hi)
    u = np.where(over, hi, np.where(under, -hi, u))
    return u, int(seen.sum()), int(over.sum() + under.sum()), int((~finite).sum())


def surface_step(frames, Ks, st, instances, subjects=None, n_subjects=None, fit_status=None, prm=None):
    """THE SURFACE STEP: RECORD_DTYPE [n_subjects]; the set's offsets, counts, points and normals after it."""
    prm = prm or params()
    n_subjects = len(st) if n_subjects is None else n_subjects
    Ks = np.asarray(Ks, dtype=np.float32)
    n = len(st.verts)
    a, b, cnt = (np.zeros((n_subjects, n), np.int64) for _ in range(3))
    e, pts_kept, used = [0] * n_subjects, [0] * n_subjects, [0] * n_subjects
    for i, inst in enumerate(instances):
        sj = 0 if subjects is None else int(subjects[i])
        if not takes_part(inst, sj, n_subjects, len(frames), None if fit_status is None else fit_status[i], st.radius, st.largest):
            continue
        f = int(inst["frame"])
        ok, J, res = instance_terms(frames[f], Ks if Ks.ndim == 2 else Ks[f], st.pts[sj], st.nrm[sj], st.nb, inst, prm)
        J, r = J[ok], res[ok]
        a[sj, ok] += np.array([int(v) for v in ((J * J) * S).tolist()], np.int64)
        b[sj, ok] += np.array([int(v) for v in ((J * r) * S).tolist()], np.int64)
        cnt[sj, ok] += 1
        e[sj] += fr._isum(r * r)
        pts_kept[sj] += int(ok.sum())
        used[sj] += 1 if ok.any() else 0
    out = np.zeros(n_subjects, RECORD_DTYPE)
    for sj in range(n_subjects):
        rec = out[sj]
        rec["points"], rec["instances"], rec["sum_r2_fixed"] = pts_kept[sj], used[sj], e[sj]
        st.counts[sj] = cnt[sj]
        if pts_kept[sj] < prm["min_points"]:
            rec["status"] = FEW_POINTS
        else:
            st.offsets[sj], rec["observed"], rec["clamped"], rec["rejected"] = solve(a[sj], b[sj], cnt[sj], st.offsets[sj], st.nbr, prm, st.max_offset)
        rec["max_abs"] = np.abs(st.offsets[sj]).max()
    st.evaluate(range(n_subjects))
    return out


def refine_subjects(frames, K, st, starts, subject_of, rounds=6, shape_rounds=0, fit_prm=None, shape_prm=None, surface_prm=None):
    """fit.refine_subjects restated: `starts` a list of instance dicts (frame, R, t, scale).  Returns (the set's state, the last
    instances, (the last round's fit records, its surface records), trace of (fit records, surface records, fitted instances) per
    round)."""
    inst = [dict(s) for s in starts]
    recs = urec = None
    trace = []
    for r in range(rounds):
        recs = []
        for s, sj in zip(inst, subject_of):
            R, t, rec = fr.fit(frames[s["frame"]], K, st.pts[sj], st.nrm[sj], s["R"], s["t"], s["scale"], fit_prm)
            s["R"], s["t"] = R, t
            recs.append(rec)
        status = [q["status"] for q in recs]
        if r < shape_rounds:
            st.update(sb.shape_step(frames, K, st, inst, subject_of, len(st), status, shape_prm))
        urec = surface_step(frames, K, st, inst, subject_of, len(st), status, surface_prm)
        trace.append((recs, urec.copy(), [dict(s) for s in inst]))
    return st.state.copy(), inst, (recs, urec), trace

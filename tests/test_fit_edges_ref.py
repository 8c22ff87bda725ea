"""The placed rows of tests/fit_edges.py on the CPU.  Each of the five restatements that carries a copy of the correspondence chain
(fit_ref, view_fit_ref, shape_ref, calib_ref, surface_ref) must give the hand-worked literals, row by row and for the aggregated
models: the only place where the five copies are compared on the compares themselves.  The table is held to its own rule too: a
local copy of the chain, which answers every link on its own, shows that each dropped row fails exactly one link, and that
relaxing one link -- `x < w` to `<=`, `y < h` to `<=`, a dropped lower bound and the rest -- keeps exactly the rows that name it
(those relaxed compares read beyond a row or a frame, so they are shown here and never run on a GPU)."""
import numpy as np
import pytest

import calib_ref as cr
import fit_edges as fe
import fit_ref as fr
import shape_ref as sr
import surface_ref as ur
import view_fit_ref as vr

F64 = np.float64
EYE = np.eye(3, dtype=F64)
GUARD = 2 * fe.W                  # elements of fe.BACK before and after the frames of the local chain's buffer


def pose(inst):
    return inst["R"].reshape(3, 3).astype(F64), inst["t"].astype(F64), F64(inst["scale"])


# ---- the five restatements, each as (points, sum_r2_fixed) of one instance
def by_fit_ref(frame, K, pts, nrm, inst, gate):
    R, t, s = pose(inst)
    _, _, e, count = fr.one_pass(frame, K, pts, nrm, s, R, t, gate)
    _, _, rec = fr.fit(frame, K, pts, nrm, R, t, s, fr.params(0, 0, (gate, gate)))
    assert (rec["points"], rec["sum_r2_fixed"], rec["steps"], rec["status"]) == (count, e, 0, fr.OK)
    return count, e


def by_view_fit_ref(frame, K, pts, nrm, inst, gate):
    R, t, s = pose(inst)
    _, _, e, count, used = vr.one_pass(frame[None], K[None], EYE[None], np.zeros((1, 3)), 0, 1, pts, nrm, s, R, t, gate)
    assert used == (1 if count else 0)
    return count, e


def by_shape_ref(frame, K, pts, nrm, inst, gate):
    basis = np.zeros((1, len(pts), 3), np.float32)
    basis[..., 2] = 1.0
    _, _, e, count = sr.instance_sums(frame, K, pts, nrm, basis, inst, gate)
    return count, e


def by_calib_ref(frame, K, pts, nrm, inst, gate):
    R, t, s = pose(inst)
    Rv, tv = vr.composite(EYE, np.zeros(3), R, t)
    _, _, e, count = cr.pair_sums(frame, K, pts, nrm, s, Rv, tv, cr.pivot_of(EYE, np.zeros(3), t), gate)
    return count, e


def by_surface_ref(frame, K, pts, nrm, inst, gate, min_cos2=0.0):
    ok, _, res = ur.instance_terms(frame, K, pts, nrm, nrm, inst, ur.params(gate=gate, min_cos2=min_cos2))
    return int(ok.sum()), fr._isum(res[ok] * res[ok])


RESTATEMENTS = {"fit_ref": by_fit_ref, "view_fit_ref": by_view_fit_ref, "shape_ref": by_shape_ref, "calib_ref": by_calib_ref,
                "surface_ref": by_surface_ref}


@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("gate", fe.GATES)
@pytest.mark.parametrize("name", sorted(RESTATEMENTS))
def test_every_restatement_gives_the_literals_row_by_row(name, gate, mirrored):
    tb = fe.per_row(gate, mirrored)
    assert len(tb.rows) == len(fe.ROWS) - 4 and tb.rows[-1].last
    for i, r in enumerate(tb.rows):
        got = RESTATEMENTS[name](tb.frames[i], tb.Ks[i], *tb.models[i], tb.inst[i], gate)
        assert got == (r.points, r.e), (name, r.name, got)


@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("n", [257, 1025])
@pytest.mark.parametrize("gate", fe.GATES)
@pytest.mark.parametrize("name", sorted(RESTATEMENTS))
def test_every_restatement_gives_the_summed_literals_on_the_aggregated_model(name, gate, n, mirrored):
    tb = fe.aggregated(n, gate, mirrored)
    assert len(tb.models[0][0]) == n and {0, 63, 64, 255, 256} <= set(tb.index.values())
    assert n == 257 or {1023, 1024} <= set(tb.index.values())
    got = RESTATEMENTS[name](tb.frames[0], tb.Ks[0], *tb.models[0], tb.inst[0], gate)
    assert got == (tb.points, tb.e), (name, got)


def test_the_literals_tell_the_kept_rows_apart():
    """Distinct g: the e of the kept rows of a table that carry one are distinct but for each gate's pair (+g and -g)."""
    for gate in fe.GATES:
        es = [r.e for r in fe.rows_of(gate, own=False) if r.e and r.gate is None]
        assert len(set(es)) == len(es) and all(e & (e - 1) == 0 for e in es)
        assert fe.aggregated(257, gate).e == sum(es) + 2 * int(gate * gate) * fe.M20


def test_the_grazing_rows_in_the_surface_restatement():
    """GRAZE * |p|^2 == c * c exactly for graze_on; the surface step keeps it and its inner neighbour and drops the outer one."""
    assert F64(fe.GRAZE) * F64(2500.0) == F64(2304.0) and (F64(0.0) + F64(14.0) * F64(14.0)) + F64(48.0) * F64(48.0) == 2500.0
    tb = fe.per_row(256.0)
    for name, want in (("graze_on", 1), ("graze_inside", 1), ("graze_outside", 0)):
        i = tb.index[name]
        assert fe.BY_NAME[name].graze == want
        assert by_surface_ref(tb.frames[i], tb.Ks[i], *tb.models[i], tb.inst[i], 256.0, fe.GRAZE) == (want, 0), name
    for n in (257, 1025):
        ag = fe.aggregated(n, 256.0, only=fe.GRAZING, graze=True)
        assert (ag.points, ag.e) == (2, 0) and sorted(ag.index.values()) == [0, 63, 64]
        assert by_surface_ref(ag.frames[0], ag.Ks[0], *ag.models[0], ag.inst[0], 256.0, fe.GRAZE) == (2, 0)
        assert by_surface_ref(ag.frames[0], ag.Ks[0], *ag.models[0], ag.inst[0], 256.0, 0.0) == (3, 0)


# ---- the table's own rule, on a local copy of the chain that answers every link on its own
def links(buf, guard, frame_index, K, v, nm, scale, R, t, gate, min_cos2=0.0):
    """{link: passes} of one point; the pixel is read as the device would read it with the frame test relaxed: (int)x, (int)y
    truncated, at frame_index * h * w + py * w + px of `buf` (the frames between `guard` elements of BACK).  A link that cannot
    be answered (the pixel of a non-finite x) is left out."""
    with np.errstate(all="ignore"):
        K = np.asarray(K, np.float32).astype(F64)
        v, nm = np.asarray(v, np.float32).astype(F64), np.asarray(nm, np.float32).astype(F64)
        sv = v * scale
        p = [((R[j, 0] * sv[0] + R[j, 1] * sv[1]) + R[j, 2] * sv[2]) + t[j] for j in range(3)]
        n = [(R[j, 0] * nm[0] + R[j, 1] * nm[1]) + R[j, 2] * nm[2] for j in range(3)]
        c = (n[0] * p[0] + n[1] * p[1]) + n[2] * p[2]
        r = [(p[0] * K[j, 0] + p[1] * K[j, 1]) + p[2] * K[j, 2] for j in range(3)]
        x, y = r[0] / r[2], r[1] / r[2]
        out = {"pz": bool(p[2] >= 1.0), "c": bool(c < 0.0), "x_lo": bool(x >= 0.0), "x_hi": bool(x < fe.W), "y_lo": bool(y >= 0.0),
               "y_hi": bool(y < fe.H), "graze": bool(c * c >= F64(min_cos2) * ((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]))}
        if np.isfinite(x) and np.isfinite(y):
            at = guard + frame_index * fe.W * fe.H + int(y) * fe.W + int(x)        # int() truncates, as the cast does
            assert 0 <= at < len(buf), "a relaxed compare would read outside the guard bands"
            d = F64(buf[at])
            out["pixel"] = bool(d != 0.0)
            out["gate"] = bool(abs(d - p[2]) <= F64(gate))
    return out


def guarded(frames):
    band = np.full(GUARD, fe.BACK, np.uint16)
    return np.concatenate([band, frames.reshape(-1), band])


def kept(lk, relaxed=()):
    return all(ok for name, ok in lk.items() if name not in relaxed)


def table_links(gate, mirrored=False, min_cos2=0.0, own=True):
    """own=False: the rows and the frame ORDER of the forms that take one K (the frame after y_equals_h is another one)."""
    tb = fe.per_row(gate, mirrored, own)
    buf = guarded(tb.frames)
    out = []
    for i, r in enumerate(tb.rows):
        R, t, s = pose(tb.inst[i])
        out.append((r, links(buf, GUARD, i, tb.Ks[i], tb.models[i][0][0], tb.models[i][1][0], s, R, t, gate, min_cos2)))
    return out


@pytest.mark.parametrize("own", [True, False])
@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("gate", fe.GATES)
def test_a_dropped_row_fails_exactly_one_link(gate, mirrored, own):
    for r, lk in table_links(gate, mirrored, own=own):
        failing = [name for name, ok in lk.items() if not ok]
        if r.K is not None and r.name in ("k_inf", "k_nan"):      # a non-finite x: the frame test alone, all of it
            assert set(failing) <= {"x_lo", "x_hi", "y_lo", "y_hi"} and r.link in failing and "pixel" not in lk, r.name
        else:
            assert failing == ([r.link] if r.link else []), (r.name, failing)
        assert kept(lk) == bool(r.points), r.name
    graze = {r.name: [name for name, ok in lk.items() if not ok] for r, lk in table_links(gate, mirrored, fe.GRAZE, own) if r.name.startswith("graze")}
    assert graze == {"graze_on": [], "graze_inside": [], "graze_outside": ["graze"]}


# what each mutant of the chain changes: the rows that a compare relaxed (or, for a kept row ON a compare, tightened) flips
RELAXED = {"pz": ["pz_below"], "c": ["c_zero"], "x_lo": ["k_negative_r2", "x_below_zero"], "x_hi": ["corner", "x_equals_w"],
           "y_lo": ["y_below_zero"], "y_hi": ["y_equals_h"], "pixel": ["pixel_zero"], "gate": ["gate%d_above_beyond", "gate%d_below_beyond"]}


@pytest.mark.parametrize("own", [True, False])
@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("gate", fe.GATES)
@pytest.mark.parametrize("link", sorted(RELAXED))
def test_relaxing_one_link_keeps_exactly_the_rows_that_name_it(link, gate, mirrored, own):
    """The mutants that may not run on a GPU (x < w to <=, y < h to <=, a dropped lower bound) among them: the corner row and
    y_equals_h are kept through the guard band past the last frame and through the next frame's first row."""
    assert set(RELAXED) | {"graze"} == set(fe.LINKS)            # (the grazing link has its own test above)
    rows = table_links(gate, mirrored, own=own)
    names = {r.name for r, _ in rows}                       # (own=False: without the rows that have a K of their own)
    flipped = sorted(r.name for r, lk in rows if not kept(lk) and kept(lk, (link,)))
    assert flipped == sorted(n for n in (n % gate if "%" in n else n for n in RELAXED[link]) if n in names)
    assert own or {"y_equals_h", "corner", "x_equals_w"} <= names
    for r, lk in rows:
        assert kept(lk) or kept(lk, (r.link,)) or r.name in ("k_inf", "k_nan"), r.name


def test_the_rows_on_a_compare_sit_on_it():
    """Each kept row that claims a compare holds the value that the compare names, exactly; the stepped rows are one f32 step off."""
    tb = fe.per_row(25.0)
    vals = {}
    for i, r in enumerate(tb.rows):
        R, t, s = pose(tb.inst[i])
        v = tb.models[i][0][0].astype(F64)
        p = v * s + t
        Kd = tb.Ks[i].astype(F64)
        with np.errstate(all="ignore"):
            rr = Kd @ p
            vals[r.name] = (p, rr[0] / rr[2], rr[1] / rr[2])
    assert vals["pz_on"][0][2] == 1.0 and vals["pixel_one"][0][2] == 1.0 and vals["pz_below"][0][2] == 1.0 - 2.0 ** -18
    assert vals["x_zero"][1] == 0.0 and vals["x_below_zero"][1] == -2.0 ** -20 and vals["x_equals_w"][1] == 16.0 and vals["corner"][1] == 16.0
    assert vals["x_below_w"][1] == 16.0 - 2.0 ** -21 and int(vals["x_below_w"][1]) == 15
    assert vals["y_zero"][2] == 0.0 and vals["y_below_zero"][2] == -2.0 ** -21 and vals["y_equals_h"][2] == 12.0
    assert vals["y_below_h"][2] == 12.0 - 2.0 ** -21 and int(vals["y_below_h"][2]) == 11 and vals["corner"][2] == 11.5
    assert vals["x_negative_zero"][1] == 0.0 and np.signbit(vals["x_negative_zero"][1]) and np.signbit(vals["x_negative_zero"][2])
    assert np.isposinf(vals["k_inf"][1]) and np.isnan(vals["k_nan"][1]) and vals["k_negative_r2"][1:] == (-8.0, 4.0)
    assert vals["gate25_above_beyond"][0][2] == 64.0 - 2.0 ** -20 and vals["gate25_below_beyond"][0][2] == 64.0 + 2.0 ** -20
    tb = fe.per_row(256.0)
    z = {name: float(tb.models[i][0][0][2]) + 64.0 for name, i in tb.index.items()}
    assert z["gate256_below_on"] == 512.0 and z["gate256_below_beyond"] == 512.0 + 2.0 ** -15 and z["gate256_above_beyond"] == 64.0 - 2.0 ** -20
    # every step is ONE f32 step: the stepped coordinate's neighbour towards the compare is the row ON it
    for name, axis, on in (("pz_below", 2, -63.0), ("x_below_zero", 0, -32.0), ("x_below_w", 0, 32.0), ("y_below_zero", 1, -24.0),
                           ("y_below_h", 1, 24.0), ("graze_inside", 1, 14.0), ("graze_outside", 1, 14.0), ("gate256_below_beyond", 2, 448.0)):
        c = np.float32(fe.BY_NAME[name].v[axis])
        assert c != np.float32(on) and np.nextafter(c, np.float32(on)) == np.float32(on), name


def test_the_mirrored_table_has_the_same_products():
    for gate in fe.GATES:
        a, b = fe.per_row(gate), fe.per_row(gate, mirrored=True)
        for (pa, _), (pb, _), ia, ib in zip(a.models, b.models, a.inst, b.inst):
            assert ib["scale"] == -0.5 and (pa.astype(F64) * F64(ia["scale"]) == pb.astype(F64) * F64(ib["scale"])).all()
        assert (a.points, a.e) == (b.points, b.e)


# ---- the aggregated model as a mesh, through the restated subject set (subjects_ref, surface_ref, ident_ref)
def field_of(n):
    B = np.zeros((1, n, 3), np.float32)
    B[..., 2] = 1.0
    return B


@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("n", [257, 1025])
@pytest.mark.parametrize("gate", fe.GATES)
def test_the_mesh_has_the_tables_normals_and_the_set_restatements_give_the_summed_literals(gate, n, mirrored):
    import ident_ref as ir
    import subjects_ref as sb
    m = fe.aggregated_mesh(n, gate, mirrored)
    tb = m.table
    assert len(m.verts) == n and m.tris.max() < n
    nrm, zero = sb.normals(m.verts, m.tris)
    assert zero == 0 and (nrm == tb.models[0][1]).all()
    plain = fe.aggregated(n, gate, mirrored)
    rows = sorted(tb.index.values())
    assert (m.verts[rows] == plain.models[0][0][rows]).all() and tb.index == plain.index
    st = sb.Set(m.verts, m.tris, field_of(n), 1)
    rec = sb.shape_step(tb.frames, fe.K, st, tb.inst, prm=sr.params(gate=gate))
    assert (rec["points"][0], rec["sum_r2_fixed"][0], rec["instances"][0]) == (tb.points, tb.e, 1)
    su = ur.Set(m.verts, m.tris, field_of(n), 1)
    rec = ur.surface_step(tb.frames, fe.K, su, tb.inst, prm=ur.params(gate=gate, min_cos2=0.0))
    assert (rec["points"][0], rec["sum_r2_fixed"][0], rec["instances"][0]) == (tb.points, tb.e, 1)
    _, _, _, scores = ir.identify(tb.frames, fe.K, st, fe.as_dicts(tb.inst), prm=ir.params(iterations=0, gate=gate))
    assert (scores["points"][0, 0], scores["sum_r2_fixed"][0, 0], scores["steps"][0, 0]) == (tb.points, tb.e, 0)


@pytest.mark.parametrize("n", [257, 1025])
def test_the_grazing_rows_as_a_mesh_in_the_restated_surface_step(n):
    m = fe.aggregated_mesh(n, 256.0, only=fe.GRAZING)
    su = ur.Set(m.verts, m.tris, field_of(n), 1)
    rec = ur.surface_step(m.table.frames, fe.K, su, m.table.inst, prm=ur.params(gate=256.0, min_cos2=fe.GRAZE))
    assert (rec["points"][0], rec["sum_r2_fixed"][0]) == (2, 0)
    rec = ur.surface_step(m.table.frames, fe.K, su, m.table.inst, prm=ur.params(gate=256.0, min_cos2=0.0))
    assert (rec["points"][0], rec["sum_r2_fixed"][0]) == (3, 0)


# ---- the tracker's start: the way the table reaches k_fit_sched
@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("n", [257, 1025])
@pytest.mark.parametrize("gate", fe.GATES)
def test_the_restated_fit_tracker_starts_from_the_tables_pose_and_carries_it(gate, n, mirrored):
    """fit_track_ref with rotation 0 and mid_point T: the first step is FITTED from the forest's pose through entry 60 of the angle
    table (cos 1, sin 0), the second CARRIED from the state; both give the summed literals and leave R = I, t = T."""
    import fit_track_ref as tr
    tb = fe.aggregated(n, gate, mirrored)
    poses, support, kw = fe.tracker_inputs()
    a = (np.arange(120) - 60.0) / 60.0 * 3.14159
    angles = np.stack([np.cos(a), np.sin(a)], axis=1)
    assert tuple(angles[60]) == (1.0, 0.0) and tr.angle_index(0.0) == 60
    ref = tr.Tracker(tb.Ks, *tb.models[0], angles, scale=float(tb.inst["scale"][0]), prm=tr.params(**kw))
    for status in (tr.FITTED, tr.CARRIED):
        rec = ref.step(tb.frames, poses, support, fit_prm=fr.params(0, 0, (gate, gate)))[0]
        assert (rec["status"], rec["fit"]["points"], rec["fit"]["sum_r2_fixed"], rec["fit"]["steps"]) == (status, tb.points, tb.e, 0)
        assert (rec["instance"]["R"].reshape(3, 3) == np.eye(3)).all() and tuple(rec["instance"]["t"]) == fe.T
        assert (ref.state["R"][0].reshape(3, 3) == np.eye(3)).all() and tuple(ref.state["t"][0]) == fe.T and ref.state["tracked"][0] == 1

"""The evaluation of DESIGN.md section 30, on the restatement alone (PYTHONPATH=. python tests/test_rig_subject_track_ref.py runs it;
some twenty seconds of numpy, which is why no test does).  The gallery is section 28's (ident_views_scenes.evaluation): three subjects
enrolled from the middle camera of the three-camera 160x120 rig, and a stranger.  Each of the four people moves as rig_fit_track_scenes.sequence moves
its head -- STEP_MM in a seeded direction and STEP_YAW degrees of yaw a step -- for 8 steps from a start none of the enrolment sets
has (view_fit_scenes.truth of 1000 * seed + 100 + salt), rendered with the sensor model through the person's own rig.  The generic
rig_fit_track_ref.Tracker and the new rule run on the same frames and the same faked persons, under the shipped defaults; per step:
mean square, position and rotation error, model used, identification.  Four starts (salt 0 - 3) say whether section 28's limit
separates known from stranger on moving frames; start 0's worst bound step is held to twice the worst of the other three."""
import functools
import math

import numpy as np

import fit_scenes as fs
import ident_ref as ir
import ident_views_scenes as ivs
import render_ref as rr
import rig_fit_track_ref as rf
import rig_fit_track_scenes as rsc
import rig_subject_track_ref as rs
import shape_scenes as ss
import view_fit_scenes as vs
from depthhead_amd import render, synth

STEPS, SALTS = 8, (0, 1, 2, 3)
ANGLES = np.array([[math.cos((i - 60) / 60.0 * 3.14159), math.sin((i - 60) / 60.0 * 3.14159)] for i in range(120)])
PEOPLE = ivs.EVAL_COEFFS + (ivs.EVAL_STRANGER,)


@functools.lru_cache(maxsize=None)
def moving(person, salt, w=160, h=120):
    """(frames [STEPS, 3, h, w], true positions [STEPS, 3], true R [STEPS, 3, 3]) of person `person` (3: the stranger) through its
    own rig of ident_views_scenes.evaluation."""
    _, _, rigs, _, _, _ = ivs.evaluation()
    Ks, V, u = rigs[person]
    key = 1000 * (ivs.EVAL_SEED + person) + 100 + salt
    pos0, R0, _ = vs.truth(key)
    un = synth.SplitMix(740000 + key).uniform(3)
    d = 2.0 * un - 1.0
    d = d / np.sqrt((d * d).sum())
    if ((pos0 + STEPS * rsc.STEP_MM * d) ** 2).sum() > (pos0 ** 2).sum():       # towards the middle of the rig
        d = -d
    sv, t, _ = ss.subject_mesh(PEOPLE[person])
    frames, pos, Rs = np.zeros((STEPS, 3, h, w), np.uint16), [], []
    for k in range(STEPS):
        p = pos0 + k * rsc.STEP_MM * d
        R = render.euler_to_matrix((0.0, rsc.STEP_YAW * k, 0.0)).astype(np.float64) @ R0
        items = [rr.instance(f, m, Rc, tc, head=hd) for f, m, Rc, tc, _, hd in vs.view_items(p, R, V, u)]
        frames[k] = rr.render([(sv, t), fs.torso()], items, 3, w, h, Ks[0], noise=2, holes=0.02, seed=key * 100 + k)[0]
        pos.append(p); Rs.append(R)
    return frames, np.stack(pos), np.stack(Rs)


def run(person, salt, ident_prm=None):
    """Per step, for the generic tracker and the new rule: (mean square mm^2, position error mm, rotation error degrees), and the
    new rule's records."""
    st, enrolled, rigs, _, _, _ = ivs.evaluation()
    Ks, V, u = rigs[person]
    v, _, n, _ = ss.generic()
    frames, pos, Rs = moving(person, salt)
    gen = rf.Tracker(Ks, V, u, [0, 3], v, n, ANGLES)
    own = rs.Tracker(Ks, V, u, [0, 3], st, (v, n), ANGLES, ident_prm=ident_prm, enrolled=enrolled)
    rows, recs = [], []
    for k in range(STEPS):
        p, hd = rsc.person(pos[k], Rs[k], V, u, 0, 0b111, k % 3, 7, 100 * person + 10 * salt + k)
        inputs = rsc.rig_inputs(3, 1, [(0, p, hd)])
        g = gen.step(frames[k], *inputs)[0, 0]
        o = own.step(frames[k], *inputs)[0, 0]
        row = []
        for r in (g, o["track"]):
            ms = r["fit"]["sum_r2_fixed"] / 1048576.0 / max(int(r["fit"]["points"]), 1)
            row.append((ms, float(np.linalg.norm(r["instance"]["t"].astype(np.float64) - pos[k])),
                        vs.geodesic_deg(r["instance"]["R"].reshape(3, 3).astype(np.float64), Rs[k])))
        rows.append(row)
        recs.append(o.copy())
    return np.array(rows), np.array(recs)


def main():
    best_known, best_stranger, bound_worst = [], [], {s: [] for s in SALTS}
    gain = []
    for salt in SALTS:
        for person in range(4):
            rows, recs = run(person, salt)
            who = "stranger" if person == 3 else f"subject {person}"
            tried = recs["identified"] == 1
            means = recs["ident"]["sum_r2_best"][tried] / 1048576.0 / np.maximum(recs["ident"]["points_best"][tried], 1)
            print(f"start {salt} {who}: identified at steps {np.flatnonzero(tried).tolist()} status {recs['ident']['status'][tried].tolist()} "
                  f"best {recs['ident']['best'][tried].astype(np.int64).tolist()} mean squares {np.round(means, 4).tolist()}")
            for k in range(STEPS):
                g, o = rows[k]
                model = int(recs["model"][k])
                print(f"    step {k}: generic ms {g[0]:7.4f} pos {g[1]:6.3f} rot {g[2]:6.3f} | own ms {o[0]:7.4f} pos {o[1]:6.3f} rot {o[2]:6.3f} "
                      f"model {'generic' if model == rs.UNKNOWN else model} status {int(recs['track']['status'][k]):#x}")
            if person < 3:
                # asserted outright: bound to themself at the first try
                assert tried[0] and recs["ident"]["status"][0] == ir.OK and recs["subject"][0] == person, (salt, person)
                assert (recs["subject"] == person).all() and (recs["model"][1:] == person).all() and tried.sum() == 1
                best_known.append(float(means[0]))
                bound = rows[1:]
                bound_worst[salt].append(bound[:, 1].max(axis=0))
                gain.append(np.stack([bound[:, 0].mean(axis=0), bound[:, 1].mean(axis=0)]))
            else:
                assert (recs["subject"] == rs.UNKNOWN).all() and (recs["model"] == rs.UNKNOWN).all(), (salt, recs["subject"])
                best_stranger += [float(m) for m in means]
    hi, lo = max(best_known), min(best_stranger)
    print(f"largest known best mean square {hi:.4f} mm^2, smallest stranger best mean square {lo:.4f} mm^2, the shipped limit 2.58^2 = {2.58 ** 2:.4f}")
    print(f"sqrt of their geometric mean {math.sqrt(math.sqrt(hi * lo)):.4f} mm")
    assert hi < 2.58 ** 2 < lo, "DH_IDENT_VIEWS_DEFAULT_MAX_RMS does not separate known from stranger on moving frames"
    gain = np.mean(gain, axis=0)
    print(f"bound steps, mean over people and starts: generic ms {gain[0, 0]:.4f} pos {gain[0, 1]:.3f} rot {gain[0, 2]:.3f} | "
          f"own ms {gain[1, 0]:.4f} pos {gain[1, 1]:.3f} rot {gain[1, 2]:.3f}")
    worst = {s: np.max(bound_worst[s], axis=0) for s in SALTS}
    others = np.max([worst[s] for s in SALTS[1:]], axis=0)
    print(f"worst bound step (ms, pos, rot): start 0 {np.round(worst[0], 4).tolist()}, starts 1 - 3 {np.round(others, 4).tolist()}")
    assert (worst[0] <= 2.0 * others).all(), "start 0's worst bound step is more than twice the other starts' worst"
    print("evaluation ok")

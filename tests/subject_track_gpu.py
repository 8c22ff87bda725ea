"""What the subject tracker's GPU tests share (test_gpu_subject_tracker.py, test_gpu_tracker_waves.py): a
tracker on the GPU beside its restated twin over one gallery and camera table, and one step of both compared byte for byte
(gpu_kit.same_records).  The device buffers of the _device forms -- uploads and guard bands -- are gpu_kit's."""
import contextlib

import fit_ref as fr
import fit_track_ref as ft
import ident_ref as ir
import subject_track_ref as stf
import subject_track_scenes as sts
from gpu_kit import same_records
from depthhead_amd import fit, tracking

# The splatted scenes are coarser than a rendered frame (tests/test_subject_track_ref.py): the identification's limit lies between a
# known head's best mean square and the stranger's, and the tracker accepts the generic head's fit of the stranger.
IDENT = dict(min_points=16, max_rms=3.8)
TRACK = dict(rms_max=8.0)


@contextlib.contextmanager
def gpu_set(name, n_subjects, surface=False):
    """(the set on the GPU, its restated twin) of ident_scenes' gallery `name`, in one state."""
    v, t, B, st = sts.restated_set(name, n_subjects, surface)
    with fit.ShapeBasis(B) as basis, fit.Subjects(v, t, basis, n_subjects, max_offset=16.0 if surface else None) as got:
        got.set_coeffs(st.state["coeffs"][:, :len(B)])
        if surface:
            for s in range(n_subjects):
                got.set_offsets(s, st.offsets[s])
        for s in (0, n_subjects - 1):
            pts, nrm = got.read(s)
            assert pts.tobytes() == st.pts[s].tobytes() and nrm.tobytes() == st.nrm[s].tobytes()
        yield got, st


@contextlib.contextmanager
def pair(angles, name, n_subjects, Ks, w, h, enrolled=None, sub=None, track=None, ident=None, surface=False, flags=0, trackers=1):
    """(trackers on the GPU, the restated tracker, the GPU set, the restated set) over one gallery and camera table."""
    track, ident = dict(TRACK if track is None else track), dict(IDENT if ident is None else ident)
    with contextlib.ExitStack() as stack:
        got, st = stack.enter_context(gpu_set(name, n_subjects, surface))
        cams = stack.enter_context(tracking.Cameras(Ks))
        model = stack.enter_context(fit.Model(*sts.generic(name)))
        trs = [stack.enter_context(fit.SubjectFitTracker(cams, got, model, w, h, motion=bool(flags), params=fit.fit_track_params(**track),
                                                         ident_params=fit.ident_params(**ident),
                                                         subject_params=None if sub is None else fit.subject_track_params(**sub), enrolled=enrolled))
               for _ in range(trackers)]
        ref = stf.Tracker(Ks, st, sts.generic(name), angles, flags=flags, prm=ft.params(**track), ident_prm=ir.params(**ident),
                          sub_prm=None if sub is None else stf.params(**sub), enrolled=enrolled)
        yield trs if trackers > 1 else trs[0], ref, got, st, cams, model


def both(tr, ref, frames, poses, sup, present=None, what="step", fit_kw=None):
    """One step on the GPU (host call) and in the restatement `ref` (anything with the restated tracker's step() and state);
    records and state compared.  fit_kw: the fit's parameters as keywords of fit.fit_params and fit_ref.params, None: the defaults."""
    got = tr.step_poses(frames, poses, sup, present, None if fit_kw is None else fit.fit_params(**fit_kw))
    want = ref.step(frames, poses, sup, present, None if fit_kw is None else fr.params(**fit_kw))
    same_records(got, want, f"records of {what}")
    same_records(tr.state(), ref.state, f"state after {what}")
    return got



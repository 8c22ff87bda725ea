"""The adversarial families of tests/edge_families.py through the vote-support restatement (tests/support_ref.py), from both
sources of taps: pyref's results (test_edge_pyref.family_results / decoy_results) and the C oracle's.

* for every 3-D family, with its own K and with its decoy cameras (ef.decoy_cameras), both sources give identical records
  at every radius of `radii`: 0, DH_SUPPORT_RADIUS, 2^31 - 1 and a boundary pair r*, r* - 1 taken from the family's own
  votes, so that the `<=` of the contract is decided on a vote;
* the families reach the edges of k_support (`assert_reach`): sums past 2^32 in both total_mass and mass, a midpoint
  saturated to INT32_MIN / INT32_MAX whose cube at r = 2^31 - 1 holds votes, and all three cases of a hit's box against
  the cube.  tests/test_gpu_support_edges.py holds the kernels to the same records and checks the same reach on them.
"""
import numpy as np
import pytest

import edge_families as ef
import support_ref as sr
from depthhead_amd import _lib
from test_edge_pyref import decoy_results, family_results

R_MAX = (1 << 31) - 1

_cache = {}


def boundary_radius(votes, mids) -> int:
    """r* of a family: the median Chebyshev distance, in [1, 2^31 - 2], of the frames' votes to their own midpoint cells
    (1 when no vote lies in that range)."""
    d = []
    for (_, _, cells, _), m in zip(votes, mids):
        if len(cells):
            c = np.max(np.abs(cells - sr.as_i32_vec(m)[None, :]), axis=1)
            d.append(c[(c >= 1) & (c < R_MAX)])
    d = np.concatenate(d) if d else np.zeros(0, np.int64)
    return int(np.sort(d)[len(d) // 2]) if len(d) else 1


def family_support(name, decoy):
    """The pyref-sourced support of a family, computed once per session: dict with frames, Ks [n, 3, 3], mids [n, 3],
    radii, recs (SUPPORT_DTYPE [len(radii), n]), votes and boxes per frame."""
    key = (name, decoy)
    if key not in _cache:
        fam, res = family_results(name)
        n = fam.frames.shape[0]
        Ks = decoy_results(name)[0] if decoy else np.repeat(np.asarray(fam.K, np.float32)[None], n, axis=0)
        if decoy:
            res = decoy_results(name)[1]
        tables = sr.LeafTables(fam.forest)
        votes = [sr.frame_votes(tables, fam.model, fam.frames[i], Ks[i], res[i]["leaf_idx"], res[i]["patch_flags"]) for i in range(n)]
        mids = np.stack([res[i]["mid_point"] for i in range(n)]).astype(np.float32)
        rs = boundary_radius(votes, mids)
        radii = [0, _lib.SUPPORT_RADIUS, R_MAX, rs, rs - 1]
        h, w = fam.frames.shape[1:]
        recs = np.zeros((len(radii), n), dtype=_lib.SUPPORT_DTYPE)
        for j, r in enumerate(radii):
            for i in range(n):
                recs[j, i] = sr.as_record(sr.support_from_votes(votes[i], mids[i], r, fam.model, w, h), _lib.SUPPORT_DTYPE)
        boxes = [sr.hit_boxes(tables, fam.model, fam.frames[i], Ks[i], res[i]["leaf_idx"], res[i]["patch_flags"]) for i in range(n)]
        _cache[key] = dict(fam=fam, frames=fam.frames, Ks=Ks, mids=mids, radii=radii, recs=recs, votes=votes, boxes=boxes)
    return _cache[key]


class Reach:
    """What the whole parametrization of the families reaches, accumulated over (family, cameras) cases."""

    def __init__(self):
        self.branches = dict.fromkeys(sr.BRANCHES, 0)
        self.total_2_32 = self.mass_2_32 = self.saturated_with_votes = 0
        self.boundary_decided = []

    def add(self, name, fs, recs):
        """`recs`: SUPPORT_DTYPE [len(radii), n] (the restatement's or the kernels')."""
        radii = fs["radii"]
        self.total_2_32 += int((recs["total_mass"] >= 1 << 32).sum())
        self.mass_2_32 += int((recs["mass"] >= 1 << 32).sum())
        jmax = radii.index(R_MAX)
        for i, m in enumerate(fs["mids"]):
            c = sr.as_i32_vec(m)
            if ((c == -(1 << 31)) | (c == R_MAX)).any() and recs[jmax, i]["mass"] > 0:
                self.saturated_with_votes += 1
            for j, r in enumerate(radii):
                for k, v in sr.branches(fs["boxes"][i], m, r).items():
                    self.branches[k] += v
        js, js1 = len(radii) - 2, len(radii) - 1
        if any(len(v[0]) for v in fs["votes"]):
            self.boundary_decided.append((name, recs[js].tobytes() != recs[js1].tobytes()))

    def check(self):
        assert self.total_2_32 > 0, "no record with total_mass >= 2^32"
        assert self.mass_2_32 > 0, "no record with mass >= 2^32"
        assert self.saturated_with_votes > 0, "no saturated midpoint whose cube at 2^31 - 1 holds votes"
        assert all(v > 0 for v in self.branches.values()), self.branches
        undecided = [n for n, d in self.boundary_decided if not d]
        assert self.boundary_decided and not undecided, ("r* and r* - 1 give the same records", undecided)


@pytest.mark.parametrize("decoy", [False, True], ids=["own_K", "decoy_cameras"])
@pytest.mark.parametrize("name", list(ef.FAMILIES))
def test_two_sources_give_identical_records(oracle, name, decoy):
    fs = family_support(name, decoy)
    fam = fs["fam"]
    tables = sr.LeafTables(fam.forest)
    for i, f in enumerate(fs["frames"]):
        mg, rg = fam.guesses(i)
        with np.errstate(all="ignore"):
            res = oracle.predict(fam.forest, fam.model, f, fs["Ks"][i], mg, rg, taps=True)
        assert np.array_equal(res.mid_point, fs["mids"][i]), (name, i)
        recs, _ = sr.replay(tables, fam.model, f, fs["Ks"][i], res.leaf_idx, res.patch_flags, res.mid_point, fs["radii"])
        for j, r in enumerate(fs["radii"]):
            assert sr.as_record(recs[j], _lib.SUPPORT_DTYPE).tobytes() == fs["recs"][j, i].tobytes(), (name, i, r, recs[j], fs["recs"][j, i])


def test_families_reach_the_support_edges():
    reach = Reach()
    for name in ef.FAMILIES:
        for decoy in (False, True):
            fs = family_support(name, decoy)
            reach.add(name, fs, fs["recs"])
    reach.check()

"""The placed scenes of tests/heads_scenes.py and the adversarial families of tests/edge_families.py through the several-heads
restatement (tests/heads_ref.py), from both sources of taps: pyref's and the C oracle's.

* for every scene, and for every 3-D family with its own K and with its decoy cameras, both sources give the same n_heads and
  the same HEAD_DTYPE bytes at every max_heads and radius the scene or family lists, and the restatement's guess cells add up
  to both sources' pos_grid;
* every scene's `reach` holds: the edge it was built for is met by the reference alone, before any kernel is compared;
* the whole parametrization reaches (`Reach.check`): frames with 0, 1, 2, 3 and 4 heads, a merged seed, a dropped zero-mass
  head, a hit supporting two heads or more, a negative centroid with a remainder, every boundary pair decided (r* against
  r* - 1, 20 against 21, 2 cells against 3) and a saturated seed coordinate; it reports, over the families, whether any has a
  saturated seed coordinate or a moment sum past 2^63 (none: DESIGN.md section 14 records why, and the placed scene
  `saturated` that stands in).
tests/test_gpu_heads_edges.py holds the kernels to the same records.
"""
import numpy as np
import pytest

import edge_families as ef
import heads_ref as hr
import heads_scenes as hs
import support_ref as sr
from depthhead_amd import _lib
from oracle import pyref

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1

_cache = {}


def scene_results(name):
    """(scene, results, infos) of a placed scene from pyref's taps, once per session; the scene's reach is checked here."""
    if name not in _cache:
        sc = hs.scene(name)
        n = len(sc.frames)
        res = [pyref.predict(sc.forest, sc.model, f, sc.K) for f in sc.frames]
        results, infos = hs.restate(sr.LeafTables(sc.forest), sc, sc.frames, [sc.K] * n,
                                    [(r["leaf_idx"], r["patch_flags"]) for r in res], sc.runs(), _lib.HEAD_DTYPE)
        for i in range(n):
            assert np.array_equal(infos[sc.runs()[0]][i]["grid"], res[i]["pos_grid"].astype(np.int64)), (name, i)
        met = sc.reach(results, infos)
        _cache[name] = (sc, results, infos, met)
    return _cache[name]


def from_oracle(oracle, tables, model, frames, Ks, runs):
    out = {}
    for mh, r in runs:
        nh = np.zeros(len(frames), np.uint32)
        recs = np.zeros((len(frames), mh), dtype=_lib.HEAD_DTYPE)
        for i, f in enumerate(frames):
            with np.errstate(all="ignore"):
                k, kept, _, _, _ = hr.heads_ref(oracle, tables, model, f, Ks[i], mh, r)     # (asserts the oracle's pos_grid)
            nh[i] = k
            recs[i] = hr.as_records(k, kept, mh, _lib.HEAD_DTYPE)
        out[(mh, r)] = (nh, recs)
    return out


def same_results(got, want, what):
    assert got.keys() == want.keys()
    for key in want:
        assert np.array_equal(got[key][0], want[key][0]), (what, key, got[key][0], want[key][0])
        assert got[key][1].tobytes() == want[key][1].tobytes(), (what, key)


class Reach:
    """What the whole parametrization reaches, accumulated over scenes and (family, cameras) cases, on the restatement's
    `infos` and on records (the restatement's or the kernels')."""
    PAIRS = ("r* against r* - 1 decided", "merged at 20, kept at 21, on x, y and z", "suppressed at 2 cells, picked at 3 (x, y, diagonal)")

    def __init__(self):
        self.head_counts = set()
        self.merged = self.dropped = self.multi = self.neg_rem = self.saturated_seed = self.past_2_63 = 0
        self.met = {}
        self.family_boundary = []

    def _infos(self, infos):
        for (mh, r), frames in infos.items():
            for info in frames:
                self.merged += info["merged"]
                self.dropped += sum(1 for c in info["candidates"] if c["support"]["mass"] == 0)
                self.multi += sum(1 for v in hs.hit_masks(info, r).values() if v & (v - 1))
                fh = info["fh"]
                for c in info["candidates"]:
                    sel = fh["g"] == c["seed_cell"]
                    sv = int(fh["vals"][sel].sum())
                    sums = [hr.exact_sum(fh["vals"][sel], fh["cells"][sel, q]) for q in range(3)]
                    self.neg_rem += any(s < 0 and s % sv for s in sums)
                    self.past_2_63 += any(abs(s) >= 1 << 63 for s in sums)
                    self.saturated_seed += any(v in (I32_MIN, I32_MAX) for v in c["seed"])

    def add_scene(self, name, results, infos, met):
        self.head_counts |= {int(v) for n, _ in results.values() for v in n}
        self._infos(infos)
        self.met.update(met)

    def add_family(self, name, decoy, fh):
        radii = fh["radii"]
        infos = {k: v for k, v in fh["infos"].items() if k[1] == radii[3]}          # (seeds and moments do not depend on r)
        self._infos(infos)
        if any(len(i["fh"]["cells"]) for i in infos[(hs.FAMILY_MAX_HEADS, radii[3])]):
            self.family_boundary.append((name, decoy, hs.differ(fh["results"], (hs.FAMILY_MAX_HEADS, radii[3]), (hs.FAMILY_MAX_HEADS, radii[4]))))

    def check(self):
        assert self.head_counts >= {0, 1, 2, 3, 4}, self.head_counts
        assert self.merged > 0, "no merged seed"
        assert self.dropped > 0, "no zero-mass head dropped"
        assert self.multi > 0, "no hit supporting two heads"
        assert self.neg_rem > 0, "no negative centroid with a remainder"
        assert self.saturated_seed > 0, "no saturated seed coordinate"
        for p in self.PAIRS:
            assert self.met.get(p), p
        assert all(self.met.values()), self.met

    def check_families(self):
        undecided = [(n, d) for n, d, ok in self.family_boundary if not ok]
        assert self.family_boundary and not undecided, ("r* and r* - 1 give the same records", undecided)


@pytest.mark.parametrize("name", list(hs.SCENES))
def test_scene_reaches_its_edge_and_both_sources_agree(oracle, name):
    sc, results, _, met = scene_results(name)
    assert met and all(met.values()), met
    got = from_oracle(oracle, sr.LeafTables(sc.forest), sc.model, sc.frames, [sc.K] * len(sc.frames), sc.runs())
    same_results(got, results, name)


@pytest.mark.parametrize("decoy", [False, True], ids=["own_K", "decoy_cameras"])
@pytest.mark.parametrize("name", list(ef.FAMILIES))
def test_family_from_both_sources(oracle, name, decoy):
    fh = hs.family_heads(name, decoy)
    got = from_oracle(oracle, fh["tables"], fh["fam"].model, fh["frames"], fh["Ks"], fh["runs"])
    same_results(got, fh["results"], (name, decoy))


def test_scenes_and_families_reach_the_heads_edges():
    reach = Reach()
    for name in hs.SCENES:
        _, results, infos, met = scene_results(name)
        reach.add_scene(name, results, infos, met)
    reach.check()
    fam = Reach()
    for name in ef.FAMILIES:
        for decoy in (False, True):
            fam.add_family(name, decoy, hs.family_heads(name, decoy))
    fam.check_families()
    print("edges met:")
    for k in sorted(reach.met):
        print("  ", k)
    print("frames with", sorted(reach.head_counts), "heads; merged seeds", reach.merged, "; zero-mass heads dropped", reach.dropped,
          "; hits supporting several heads", reach.multi, "; negative centroids with a remainder", reach.neg_rem)
    print("families: saturated seed coordinates", fam.saturated_seed, "; moment sums past 2^63:", fam.past_2_63,
          "; merged", fam.merged, "; head counts", sorted({int(v) for n in ef.FAMILIES for d in (False, True)
                                                           for nh, _ in hs.family_heads(n, d)["results"].values() for v in nh}))
    # what DESIGN.md section 14 records about the families; a change of the families that changes it has to change it there
    assert fam.past_2_63 == 0, "a family's moment sum passes 2^63: DESIGN.md section 14 says none does"
    assert fam.saturated_seed == 0, "a family now has a saturated seed coordinate: DESIGN.md section 14 says only the placed scene does"

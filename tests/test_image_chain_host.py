"""CPU half of the frame image chain's checks on stamped images (tests/image_chain_cases.py): the vectorised restatement equals the
literal per-pixel functions of tests/golden/make_golden.py bit for bit on small images of every family, the oracle equals the
restatement on every case at full size, and every premise the GPU cases rest on (which seam, tile, pass or controller branch a case
reaches) is asserted from the restatement and `classify` alone.  A premise that fails is a failed test."""
import numpy as np
import pytest

import image_chain_cases as ic
from golden import make_golden as mg


# ---- the vectorised restatement against the literal functions -----------------------------------------------------------------------------
def literal_chain(img, cfg, thresholds, max_described=None):
    """image_chain_ref spelled with the per-pixel literals: fast9_16 per region on the sub-image, border filter, brief32 /
    orb_describe_ref per keypoint (the first max_described only: they take milliseconds each)."""
    rows, cols = cfg["rows"], cfg["cols"]
    kps, raw = [], []
    for (rx, ry, rw, rh), t in zip(ic.cfg_regions(cfg), thresholds):
        found = mg.fast9_16(img[ry:ry + rh, rx:rx + rw], t)
        raw.append(len(found))
        kps += [(x + rx, y + ry, s) for x, y, s in found]
    b = ic.BORDER[cfg["extractor"]]
    kps = sorted([k for k in kps if b <= k[0] < cols - b and b <= k[1] < rows - b], key=lambda k: (k[1], k[0]))
    if cfg["extractor"] == ic.ORB:
        blur, pat = mg.gaussian_blur7_ref(img), mg.read_orb_pattern()
        desc = [mg.orb_describe_ref(blur, x, y, -1.0, pat) for x, y, _ in kps[:max_described]]
    else:
        pat = mg.read_brief_pattern()
        desc = [mg.brief32(img, x, y, pat) for x, y, _ in kps[:max_described]]
    return np.array([k[:2] for k in kps], np.int16).reshape(-1, 2), np.array([k[2] for k in kps], np.int32), np.array(desc, np.uint8).reshape(-1, 32), raw


def _small_families():
    fam = {}
    pts = ic.place(ic.lattice(3, 147, 3, 97, 5))
    fam["stamps"] = (ic.stamps(100, 150, pts, seed=1), ic.make_cfg(100, 150), [20])
    fam["stamps-orb"] = (ic.stamps(100, 150, pts, seed=2), ic.make_cfg(100, 150, extractor=ic.ORB), [20])
    for t in (1, 40, 254):
        fam["saturated-%d" % t] = (ic.saturated_noise(64, 96, seed=3), ic.make_cfg(64, 96), [t])
    cv = ic.Canvas(100, 131, seed=4)
    ic.plateau_pairs(cv, [((63, 20 + 14 * i), (1, (i % 3) - 1), ("equal", "first", "second")[i // 3]) for i in range(5)] + [((63, 63), (1, 1), "equal")])
    ic.arc_stamps(cv, ic.lattice(6, 128, 6, 97, 12), 20)
    fam["arcs-pairs"] = (cv.img, ic.make_cfg(100, 131), [20])
    c = ic.case("regions-2x3-100x150")
    fam["grid-2x3"] = (c["frames"][1][0], c["cfg"], ic.ref_of("regions-2x3-100x150")[1]["thr_in"])
    fam["grid-2x3-orb"] = (c["frames"][2][1], dict(c["cfg"], extractor=ic.ORB), [20, 33, 21, 30, 25, 40])
    sat = ic.case("fast_saturation-254")
    fam["extremes-254"] = (sat["frames"][0][0], sat["cfg"], [254])
    return fam


SMALL = _small_families()


@pytest.mark.parametrize("name", list(SMALL))
def test_vectorised_restatement_equals_the_literal_functions(name):
    img, cfg, thr = SMALL[name]
    got = ic.image_chain_ref(img, cfg, thr)
    xy, score, desc, raw = literal_chain(img, cfg, thr, max_described=60)
    assert got["raw"] == raw
    np.testing.assert_array_equal(got["xy"], xy)
    np.testing.assert_array_equal(got["score"], score)
    np.testing.assert_array_equal(got["desc"][:len(desc)], desc)
    if name in ("stamps", "stamps-orb", "arcs-pairs", "grid-2x3", "grid-2x3-orb"):
        assert len(desc) >= 20 and sum(raw) > len(xy) > 0, (len(desc), raw)            # the comparison is not empty


def test_vectorised_fast_equals_the_fast_fixture(golden):
    """fast.npz was written by fast9_16: blob, edge, L corner, plateau, 8- and 9-arc, block images, noise, at three thresholds, and
    the region form."""
    g = golden["fast"]
    names = [k[4:] for k in g.files if k.startswith("img_") and k != "img_roi"]
    assert len(names) >= 9
    for name in names:
        for thr in (10, 20, 50):
            x, y, s = ic.fast_ref(g["img_" + name], thr)
            np.testing.assert_array_equal(np.stack([x, y, s], axis=1), g["kp_%s_%d" % (name, thr)], err_msg="%s %d" % (name, thr))
    rx, ry, rw, rh = [int(v) for v in g["roi"]]
    x, y, s = ic.fast_ref(g["img_roi"][ry:ry + rh, rx:rx + rw], 20)
    np.testing.assert_array_equal(np.stack([x, y, s], axis=1), g["kp_roi_20"])


def test_controller_restatement_equals_the_controller_fixture(golden):
    g = golden["controller"]
    cfg = ic.make_cfg(376, 1241)
    assert ic.target_per_detector(cfg) == int(g["target"])
    thr = [cfg["thr_min"]]
    for (cl, cr), want in zip(g["counts"], g["thresholds"]):
        thr = ic.controller_ref(thr, [int(cl)], [int(cr)], cfg)
        assert thr == [int(want)]


def test_regions_are_disjoint_with_a_gap_between_neighbours():
    """Independent of derive_cfg's arithmetic: the evaluated areas of a grid are disjoint, lie inside the image, and neighbours are
    two pixels apart (three where the cell size is fractional)."""
    for rows, cols, det in ((130, 200, (2, 2)), (130, 200, (1, 3)), (100, 150, (2, 3)), (200, 333, (4, 4)), (376, 1241, (1, 1)), (200, 1100, (1, 3))):
        regs = ic.regions(rows, cols, *det)
        seen = np.zeros((rows, cols), np.int32)
        for reg in regs:
            x0, x1, y0, y1 = ic.valid_area(reg)
            assert 3 <= x0 < x1 <= cols - 3 and 3 <= y0 < y1 <= rows - 3, (reg, rows, cols)
            seen[y0:y1, x0:x1] += 1
        assert seen.max() == 1
        gaps_x = np.diff(np.nonzero(seen.any(axis=0))[0])
        gaps_y = np.diff(np.nonzero(seen.any(axis=1))[0])
        # two columns between neighbours; three where the cell width is no whole number (the width is truncated, the origin rounded)
        assert set(gaps_x) <= {1, 3, 4} and set(gaps_y) <= {1, 3, 4}
        assert (gaps_x > 1).sum() == det[1] - 1 and (gaps_y > 1).sum() == det[0] - 1
        if rows % det[0] == 0 and cols % det[1] == 0:
            assert set(gaps_x) <= {1, 3} and set(gaps_y) <= {1, 3}


# ---- the oracle against the restatement, every case at full size ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ic.CASES)
def test_oracle_equals_the_restatement(name):
    cfg = ic.case(name)["cfg"]
    for k, (rec, want) in enumerate(zip(ic.oracle_of(name), ic.ref_of(name))):
        ic.assert_image_chain(rec, 0, want, cfg, "%s frame %d" % (name, k))


# ---- premises -----------------------------------------------------------------------------------------------------------------------------
def _has(xy, p):
    return bool(((xy[:, 0] == p[0]) & (xy[:, 1] == p[1])).any())


FAST_SEAMS = [n for n in ic.CASES if n.startswith("fast_seams")]


@pytest.mark.parametrize("name", FAST_SEAMS)
def test_premises_fast_seams(name):
    c = ic.case(name)
    cfg = c["cfg"]
    cols = cfg["cols"]
    kinds = {}
    for side in (0, 1):
        _fast_seams_side(c, side, kinds)
    # every rotation and sign of each arc kind is drawn (the narrow images share them between left and right)
    assert all(len(kinds[k]) == 32 for k in ("nine", "eight", "nine_t")), {k: len(v) for k, v in kinds.items()}
    staging = set(ic.classify(cfg, c["stride"])["staging"].values())
    assert staging == ({"byte"} if cols == 131 or c["stride"] % 4 else {"byte", "dword"}), (name, staging)
    tx_last = ic.classify(cfg)["TX"] - 1
    assert cols - tx_last * 64 == {131: 3, 132: 4, 193: 1, 257: 1, 333: 13}[cols]          # 193 and 257: a last tile one pixel wide
    assert not np.array_equal(c["frames"][0][0], c["frames"][0][1])


def _fast_seams_side(c, side, kinds):
    cfg, meta = c["cfg"], c["meta"][side]
    cols, rows, t = cfg["cols"], cfg["rows"], cfg["thr_min"]
    got = ic.ref_of(c["name"])[0]["sides"][side]
    raw = got["raw_xy"]
    # plateau pairs: neither pixel of an equal pair survives, the weaker pixel of an unequal pair dies alone
    crossed = set()
    for (x, y), (dx, dy), flavour in meta["pairs"]:
        p, q = _has(raw, (x, y)), _has(raw, (x + dx, y + dy))
        assert (p, q) == {"equal": (False, False), "first": (True, False), "second": (False, True)}[flavour], ((x, y), (dx, dy), flavour)
        for seam in (63, 127):
            if flavour == "equal" and min(x, x + dx) == seam and dx:
                crossed.add(("column", seam, dy * dx))
            if flavour == "equal" and min(y, y + dy) == seam and dy:
                crossed.add(("row", seam, dx * dy))
    column_seams = [a for a in (63, 127) if a + 1 <= cols - 4]
    for a in column_seams:
        assert {("column", a, g) for g in (-1, 0, 1)} <= crossed, (a, crossed)
    for a in (63, 127):
        assert {("row", a, g) for g in (-1, 0, 1)} <= crossed, (a, crossed)
    if cols == 333:
        assert len(column_seams) == 2 and sum(1 for (x, y), d, f in meta["pairs"] if f == "equal" and x in (63, 64, 127, 128) and y in (63, 64, 127)) == 4
    # arcs: every rotation and sign of the exact 9-arc is kept with score t, every 8-arc and every 9-arc with one pixel at t is absent
    for x, y, kind in meta["arcs"]:
        kinds.setdefault(kind[2], set()).add(kind[:2])
        hit = (raw[:, 0] == x) & (raw[:, 1] == y)
        if kind[2] == "nine":
            assert hit.sum() == 1 and got["raw_score"][hit][0] == t, (x, y, kind)
        else:
            assert not hit.any(), (x, y, kind)
    # the last pixel FAST evaluates and the first it does not, on all four sides
    on = {"right": 0, "bottom": 0, "left": 0, "top": 0}
    for x, y in meta["edge"]:
        inside = 3 <= x <= cols - 4 and 3 <= y <= rows - 4
        assert _has(raw, (x, y)) == inside, (x, y)
        for where, cond in (("right", x == cols - 4), ("bottom", y == rows - 4), ("left", x == 3), ("top", y == 3)):
            on[where] += int(cond)
    assert all(on.values()) and sum(1 for x, y in meta["edge"] if x in (2, cols - 3) or y in (2, rows - 3)) >= 4, on


def test_premises_fast_saturation():
    walk = ic.ref_of("fast_saturation-1-255")
    assert [f["thr_in"] for f in walk] == [[1], [2], [4]] and walk[2]["thr_after"] == [8]
    for name, n_extreme in (("fast_saturation-1-255", 4), ("fast_saturation-254", 4), ("fast_saturation-255", 0)):
        c = ic.case(name)
        for k, f in enumerate(ic.ref_of(name)):
            for side in (0, 1):
                img = c["frames"][k][side]
                assert (img == 0).mean() > 0.2 and (img == 255).mean() > 0.2        # v - t < 0 and v + t > 255 at every threshold
                assert (f["sides"][side]["score"] == 254).sum() >= n_extreme
                if name == "fast_saturation-255":
                    assert len(f["sides"][side]["raw_xy"]) == 0
                if name == "fast_saturation-254":
                    assert len(f["sides"][side]["xy"]) > 0 and (f["sides"][side]["raw_score"] == 254).all()


REGION_CASES = [n for n in ic.CASES if n.startswith("regions-")]


@pytest.mark.parametrize("name", REGION_CASES)
def test_premises_regions(name):
    c = ic.case(name)
    cfg = c["cfg"]
    ref = ic.ref_of(name)
    assert len(set(ref[1]["thr_in"])) > 1 and len(set(ref[2]["thr_in"])) > 1, ref[1]["thr_in"]           # unequal thresholds in effect
    branches = set(ic.classify(cfg)["branch"].values())
    assert {"clipped", "per_pixel"} <= branches, branches
    # stamps on the first / last evaluated pixel of every region edge are found, those one pixel outside (the gap) are not
    areas = [ic.valid_area(r) for r in ic.cfg_regions(cfg)]
    drawn = ic.place(c["meta"]["edge"])
    n_in = n_out = 0
    for k in (1, 2):
        raw = ref[k]["sides"][0]["raw_xy"]
        for x, y in drawn:
            inside = any(x0 <= x < x1 and y0 <= y < y1 for x0, x1, y0, y1 in areas)
            assert c["frames"][k][0][y, x] == 220 and _has(raw, (x, y)) == inside, (x, y, inside)
            n_in += inside; n_out += not inside
    assert n_in >= 4 * len(areas) and n_out >= 4 * len(areas), (n_in, n_out)


def test_premises_regions_reach_all_three_threshold_branches():
    """A tile takes the uniform-threshold form without clipping only if its 66 x 66 score region lies inside ONE region's evaluated area:
    that takes a region of 72 rows at the least and a tile row that is neither the first nor the last, which none of the 130-, 100- and
    200-row grids has.  regions-1x2-200x333 has such tiles; the others reach the clipped and the per-pixel form."""
    seen = {}
    for name in REGION_CASES:
        seen[name] = set(ic.classify(ic.case(name)["cfg"])["branch"].values())
    assert seen["regions-1x2-200x333"] == {"uni_full", "clipped", "per_pixel"}, seen
    assert set.union(*seen.values()) == {"uni_full", "clipped", "per_pixel"}


def test_premises_controller_edges():
    trace = set()
    for name, plan in (("controller_edges-1x1", ic.CONTROLLER_PLAN_1X1), ("controller_edges-2x2", ic.CONTROLLER_PLAN_2X2)):
        c = ic.case(name)
        cfg = c["cfg"]
        T, tol = ic.target_per_detector(cfg), cfg["tol"]
        lo, hi = round(T * (1 - tol), 9), round(T * (1 + tol), 9)
        assert lo == int(lo) and hi == int(hi)                                   # the tolerance band ends on whole counts
        counts = [n for frame in plan for pair in frame for n in pair]
        assert {T, int(lo), int(lo) - 1, int(hi), int(hi) + 1} <= set(counts), (T, counts)
        thr = [cfg["thr_min"]] * len(plan[0])
        for k, f in enumerate(ic.ref_of(name)):
            assert f["sides"][0]["raw"] == [p[0] for p in plan[k]] and f["sides"][1]["raw"] == [p[1] for p in plan[k]], (name, k)
            assert any(a != b for a, b in plan[k])
            thr = ic.controller_ref(thr, f["sides"][0]["raw"], f["sides"][1]["raw"], cfg, trace)
            assert thr == f["thr_after"]
    assert trace == set(ic.CONTROLLER_BRANCHES), set(ic.CONTROLLER_BRANCHES) - trace
    # the counts exactly on the band's ends change nothing
    cfg = ic.case("controller_edges-1x1")["cfg"]
    assert ic.controller_ref([6], [135], [165], cfg) == [6] and ic.controller_ref([6], [134], [134], cfg) != [6]


EMIT = {"emit_passes-200x1100": dict(TX=18, passes=2, seams=[(113, 14)], q64=3, r64=10),
        # 64 x 4160 is 4160 words: a third pass of 64 words, which starts in row 63 (no keypoint there: the border)
        "emit_passes-64x4160": dict(TX=65, passes=3, seams=[(31, 33), (63, 1)], q64=0, r64=64),
        "emit_passes-376x1241": dict(TX=20, passes=4, seams=[(102, 8), (204, 16), (307, 4)], q64=3, r64=4),
        "emit_passes-64x64": dict(TX=1, passes=1, seams=[], q64=64, r64=0),
        "emit_passes-70x65": dict(TX=2, passes=1, seams=[], q64=32, r64=0)}


@pytest.mark.parametrize("name", [n for n in ic.CASES if n.startswith("emit_passes")])
def test_premises_emit_passes(name):
    c = ic.case(name)
    cfg = c["cfg"]
    want = EMIT[name.replace("-orb", "")]
    cl = ic.classify(cfg)
    assert {k: cl[k] for k in want} == want
    ref = ic.ref_of(name)[0]
    b = ic.BORDER[cfg["extractor"]]
    for side in (0, 1):
        xy = ref["sides"][side]["xy"]
        in_passes = sorted(set(ic.emit_pass_of(xy, cfg)))
        assert in_passes == list(range(want["passes"] if "64x4160" not in name else 2)) and (len(in_passes) >= 2 or not want["seams"])
        for row, word in want["seams"]:
            if not b <= row < cfg["rows"] - b:
                continue
            in_row = xy[xy[:, 1] == row][:, 0] // 64
            assert (in_row == word - 1).any() and (in_row == word).any() and (in_row < word - 1).any() and (in_row > word).any(), (row, word)
        assert not np.array_equal(c["frames"][0][0], c["frames"][0][1])
    # kept and dropped stamps on every side of the border: left / right in the left image, top / bottom in the right one
    if min(cfg["rows"], cfg["cols"]) - 2 * b >= 8:
        for side in (0, 1):
            pts, at = c["meta"]["border"][side]
            s = ref["sides"][side]
            n = (cfg["cols"], cfg["rows"])[side]
            assert at == (b - 1, b, n - b - 1, n - b)
            for p in pts:
                assert _has(s["raw_xy"], p), p                                               # every one of them is a detection ...
                assert _has(s["xy"], p) == (b <= p[side] < n - b), p                         # ... and the border decides
            assert {p[side] for p in pts} == set(at)
    else:
        assert sum(len(ref["sides"][side]["xy"]) for side in (0, 1)) >= 2 and ref["n_detected"][0] > 100


BRIEF_CASES = [n for n in ic.CASES if n.startswith("brief_tiles")]


@pytest.mark.parametrize("name", BRIEF_CASES)
def test_premises_brief_tiles(name):
    c = ic.case(name)
    cfg = c["cfg"]
    b = ic.BORDER[cfg["extractor"]]
    ref = ic.ref_of(name)[0]
    for side in (0, 1):
        s = ref["sides"][side]
        xy, desc = s["xy"], s["desc"]
        # descriptors: no two neighbours of the list alike, 95 % unique overall (a keypoint given another's descriptor would show)
        assert (desc[1:] != desc[:-1]).any(axis=1).all()
        assert len(np.unique(desc, axis=0)) >= 0.95 * len(desc), (len(np.unique(desc, axis=0)), len(desc))
        counts = ic.brief_tile_counts(xy, cfg)
        if "200x400" in name:
            for tile, want in ic.BRIEF_TILE_PLAN.items():
                assert counts.get(tile, 0) == want, (tile, counts.get(tile, 0), want)
            tx, ty = ic.BRIEF_TILE_ONE_ROW
            one = xy[(xy[:, 0] // 128 == tx) & (xy[:, 1] // 64 == ty)]
            assert len(one) >= 20 and len(set(one[:, 1])) == 1
            tx, ty = ic.BRIEF_TILE_TWO_ROWS
            two = xy[(xy[:, 0] // 128 == tx) & (xy[:, 1] // 64 == ty)]
            assert set(two[:, 1] % 64) == {0, 63} and min((two[:, 1] % 64 == 0).sum(), (two[:, 1] % 64 == 63).sum()) >= 20
            assert all((xy[:, 0] == v).any() for v in (127, 128)) and all((xy[:, 1] == v).any() for v in (63, 64))
            assert ic.classify(cfg)["TX"] * 64 > cfg["cols"]
        else:
            edge = c["meta"]["edge_x"]
            assert edge == cfg["cols"] - b - 1 and (xy[:, 0] == edge).sum() >= 20
            tx = edge // 128
            assert tx * 128 - 24 + 176 > ic.classify(cfg)["bstride"]               # the tile's staged region runs past the padded row
            assert (ic.classify(cfg)["bstride"] == cfg["cols"]) == ("200x384" in name)
            assert max(counts.values()) > 256
    assert not np.array_equal(c["frames"][0][0], c["frames"][0][1])


def test_premises_overflow_and_streams():
    for cap in (100, 257):
        c = ic.overflow_case(cap)
        ref = ic.run_ref(c)[0]
        assert [len(s["xy"]) for s in ref["sides"]] == [435, 435] and ref["n_detected"] == [975, 975] and cap < 435
    seeds = list(range(9))
    firsts = [ic.stream_case(s)["frames"][0][0] for s in seeds]
    assert all(not np.array_equal(firsts[i], firsts[j]) for i in seeds for j in seeds if i < j)
    ref = ic.run_ref(ic.stream_case(1))
    assert len(set(ref[1]["thr_in"])) >= 1 and all(len(f["sides"][0]["xy"]) > 100 for f in ref)

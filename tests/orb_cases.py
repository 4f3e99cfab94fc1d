"""What the OrbDetector sweep shares (test_orb_sweep_host.py on the CPU, test_orb_sweep_gpu.py on the GPU): the images, a
restatement of the whole detector, the case list and the premises each case must meet.

No fixtures, no GPU use, nothing random beyond numpy.random.default_rng(seed).

The restatement `orb_detect_ref` is put together from the pinned pieces of tests/golden/make_golden.py, imported and not copied:
resize_linear_ref, harris_ref, ic_angle_ref, orb_umax_ref, retain_best_ref.  What joins them is restated here in Python: the
per-level quotas, the pyramid and the rule that ends it, the border filter, both retainBest steps, the level order and the
scale-back.  The C entry takes the scale factor as a float, so the quotas start from float32(scale_factor), and a level's size is
cvRound of the FLOAT quotient rows / scale as orb.cpp writes it (`same_level_sizes` shows that the double quotient of
make_golden.orb_detect_ref gives the same sizes in every case here).

FAST is an argument, `fast(level_image, threshold) -> [(x, y, score)]`:
  make_golden.fast9_16   the scalar Python double loop: fully independent, affordable up to roughly 150 x 190 (family g);
  oracle_fast(oracle)    the oracle's stand-alone FAST entry on the restatement's OWN level image.  Then the restatement leans on
                         the oracle's FAST alone, which is pinned elsewhere (fast.npz, thirteen shapes in
                         test_hip_random_shapes.py); everything behind FAST stays independent of the oracle.
The pinned pieces are pure functions of a level image, so their results are kept per image (`_memo`): the families reuse three
images, and a budget chosen from a probe run costs the probe only once.

Beside the keypoints the restatement returns one record per level it ran: the corners inside the border, what each retainBest
kept, the response and the class size at each cut, and the responses and keep masks in input order.  The premises read only these,
never the code under test.  A parameter that a premise depends on is searched in a fixed order and the misses are counted
(`Case.rejected`); no case skips."""
import functools
import hashlib

import numpy as np

from golden import make_golden as mg

SEED, CELL = 5, 4
THR, EDGE, PATCH = 20, 31, 31
SEAM = 1024                  # k_orb_select compacts in sweeps of 1024; its 8-bit branch and the float branch share that loop
LARGE, SMALL = (240, 400), (100, 130)

_memo = {}


def _memoized(tag, lev, rest, make):
    key = (tag, lev.shape, hashlib.sha1(lev.tobytes()).digest()) + rest
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


@functools.lru_cache(maxsize=None)
def oracle_fast(api):
    """FAST-9/16 + NMS of the stand-alone entry (CApi.fast_detect) as a `fast` argument."""
    def fast(lev, thr):
        xy, score = api.fast_detect(lev, (0, 0, lev.shape[1], lev.shape[0]), thr)
        return [(int(x), int(y), int(s)) for (x, y), s in zip(xy, score)]
    return fast


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def level_quotas(nfeatures, scale_factor, nlevels):
    """orb.cpp computeKeyPoints: nfeaturesPerLevel, float arithmetic, the last level takes the rest."""
    f = np.float32
    factor = f(1.0 / float(f(scale_factor)))
    nd = f(nfeatures) * (f(1) - factor) / (f(1) - f(np.power(float(factor), float(nlevels))))
    per, total = [], 0
    for _ in range(nlevels - 1):
        per.append(int(np.rint(nd)))
        total += per[-1]
        nd = f(nd * factor)
    per.append(max(nfeatures - total, 0))
    return per


def level_sizes(rows, cols, scale_factor, nlevels, edge, double_quotient=False):
    """(level, scale, rows, cols) of every level that runs: a level on which nothing can survive the border filter ends the pyramid."""
    f = np.float32
    out = []
    for l in range(nlevels):
        sc = f(np.power(float(f(scale_factor)), float(l)))
        if l == 0:
            out.append((0, sc, rows, cols))
            continue
        if double_quotient:
            nr, nc = int(np.rint(rows / float(sc))), int(np.rint(cols / float(sc)))
        else:
            nr, nc = int(np.rint(f(rows) / sc)), int(np.rint(f(cols) / sc))
        if nr < 2 * edge + 8 or nc < 2 * edge + 8:
            break
        out.append((l, sc, nr, nc))
    return out


def _select(resp, n):
    """retainBest(n) over responses in input order: keep mask, the response at the cut and the size of its class (None: no cut)."""
    kept = mg.retain_best_ref([dict(i=i, response=r) for i, r in enumerate(resp)], n)
    keep = np.zeros(len(resp), bool)
    keep[[k["i"] for k in kept]] = True
    if not 0 < n < len(resp):
        return keep, None, None
    cut = np.sort(resp)[::-1][n - 1]
    return keep, cut, int((resp == cut).sum())


def orb_detect_ref(img, nfeatures, scale_factor, nlevels, edge, patch, fast_thr, fast=mg.fast9_16):
    """-> (keypoints [n, 6] float32 as vslam_orb_detect writes them, one record per level that ran)."""
    f = np.float32
    per = level_quotas(nfeatures, scale_factor, nlevels)
    half = patch // 2
    umax = mg.orb_umax_ref(half)
    lev = np.ascontiguousarray(img, np.uint8)
    out, levels = [], []
    for l, sc, nr, nc in level_sizes(img.shape[0], img.shape[1], scale_factor, nlevels, edge):
        if l > 0:
            lev = _memoized("resize", lev, (nr, nc), functools.partial(mg.resize_linear_ref, lev, nr, nc))
        pts = _memoized("fast", lev, (fast, fast_thr), functools.partial(fast, lev, fast_thr))
        pts = [(x, y, s) for (x, y, s) in pts if edge <= x < nc - edge and edge <= y < nr - edge]          # runByImageBorder
        score = np.array([s for _, _, s in pts], np.float32)
        keep1, cut1, class1 = _select(score, 2 * per[l])                                                   # retainBest(2 n) on the FAST score
        pts1 = [p for p, k in zip(pts, keep1) if k]
        harris = np.array([_memoized("harris", lev, (x, y), functools.partial(mg.harris_ref, lev, x, y)) for x, y, _ in pts1], np.float32)
        keep2, cut2, class2 = _select(harris, per[l])                                                      # retainBest(n) on the Harris response
        for (x, y, _), r, k in zip(pts1, harris, keep2):
            if k:
                ang = _memoized("angle", lev, (x, y, half), functools.partial(mg.ic_angle_ref, lev, x, y, half, umax))
                out.append([f(x) * sc if l else f(x), f(y) * sc if l else f(y), f(patch) * sc, ang, r, f(l)])
        levels.append(dict(level=l, rows=nr, cols=nc, quota=per[l], n_border=len(pts), n1=len(pts1), n2=int(keep2.sum()), cut1=cut1, class1=class1,
                           cut2=cut2, class2=class2, score=score, keep1=keep1, harris=harris, keep2=keep2))
    return np.array(out, np.float32).reshape(-1, 6), levels


def same_level_sizes(case):
    a = level_sizes(case.img.shape[0], case.img.shape[1], case.scale_factor, case.nlevels, case.edge)
    return a == level_sizes(case.img.shape[0], case.img.shape[1], case.scale_factor, case.nlevels, case.edge, double_quotient=True)


def same_rows(a, b):
    """bit for bit, rows in order"""
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- images ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def block_image(rows, cols, seed=SEED):
    """blocks of random grey, cells of 4 px, noise +-3: corners at the junctions, no plateau for the suppression to empty"""
    img = mg.block_image(np.random.default_rng(seed), rows, cols, CELL)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def periodic_image(tile=32, ny=8, nx=13, seed=SEED):
    """one block-plus-noise tile repeated: every corner away from the frame recurs with the same 9 x 9 neighbourhood, so Harris
    responses fall into classes of ny x nx (less what the border takes) equal values"""
    img = np.tile(mg.block_image(np.random.default_rng(seed), tile, tile, CELL), (ny, nx))
    img.setflags(write=False)
    return img


def strided_view(img, pad=5, lead=3, fill=255):
    """the image inside a wider buffer, as the RGB-D tracker hands a detector region of its grid to the entry"""
    rows, cols = img.shape
    stride = cols + pad
    buf = np.full(lead + rows * stride, fill, np.uint8)
    view = buf[lead:].reshape(rows, stride)[:, :cols]
    view[...] = img
    return view


# ---- cases -------------------------------------------------------------------------------------------------------------------------
class Case(object):
    def __init__(self, name, img, nfeatures, scale_factor=1.2, nlevels=1, edge=EDGE, patch=PATCH, thr=THR, python_fast=False, strided=False,
                 premise=None, rejected=0, seed=SEED):
        self.name, self.family, self.img, self.seed = name, name[0], img, seed
        self.nfeatures, self.scale_factor, self.nlevels, self.edge, self.patch, self.thr = int(nfeatures), scale_factor, nlevels, edge, patch, thr
        self.python_fast, self.strided, self.premise, self.rejected = python_fast, strided, premise, rejected

    @property
    def args(self):
        return (self.nfeatures, self.scale_factor, self.nlevels, self.edge, self.patch, self.thr)

    def __repr__(self):
        return "%s: %d x %d (seed %d), nfeatures %d, factor %g, %d levels, edge %d, patch %d, threshold %d%s" % (
            (self.name,) + self.img.shape + (self.seed,) + self.args + (", strided" if self.strided else "",))


def reference(case, fast):
    """the restatement's (keypoints, levels) of a case; `fast` is ignored where the case asks for the Python FAST"""
    fast = mg.fast9_16 if case.python_fast else fast
    return _memoized("case", case.img, case.args + (fast,), lambda: orb_detect_ref(case.img, *case.args, fast=fast))


def detect(api, case, cap=20000):
    if case.strided:
        view = strided_view(case.img)
        return api.orb_detect(view, *case.args, cap=cap, row_stride=view.strides[0])
    return api.orb_detect(case.img, *case.args, cap=cap)


def describe(levels):
    def num(v):
        return "-" if v is None else "%.9g" % v
    return "; ".join("L%d %dx%d quota %d: border %d, first %d (cut %s, class %s), second %d (cut %s, class %s)" % (
        L["level"], L["rows"], L["cols"], L["quota"], L["n_border"], L["n1"], num(L["cut1"]), L["class1"], L["n2"], num(L["cut2"]), L["class2"])
        for L in levels)


def _classes(resp):
    """distinct responses, largest first, and the number of corners at or above each"""
    vals, counts = np.unique(resp, return_counts=True)
    return vals[::-1], np.cumsum(counts[::-1])


def _both_sides(idx, n):
    """members of a kept / dropped set before and behind the first seam of the compaction"""
    return n > SEAM and idx[:SEAM].any() and idx[SEAM:].any()


# a. seams of the select ---------------------------------------------------------------------------------------------------------------
def _seam_search(img, fast, target):
    """every (edge, threshold, budget) for which the first select hands exactly `target` corners to the second.  Up to the seam only
    sets whose corners inside the border are that many, so that neither select sweeps twice; behind it also those whose FAST scores
    have a class that ends at `target` and an even 2 * budget inside it."""
    rows, cols = img.shape
    for thr in (20, 19, 21, 18, 22, 17, 23, 16, 24):
        pts = np.array(_memoized("fast", img, (fast, thr), functools.partial(fast, img, thr)), np.int64).reshape(-1, 3)
        for edge in range(EDGE, 100):
            score = pts[(pts[:, 0] >= edge) & (pts[:, 0] < cols - edge) & (pts[:, 1] >= edge) & (pts[:, 1] < rows - edge), 2]
            if len(score) < target:
                break
            if len(score) == target:
                yield edge, thr, (target + 1) // 2
            elif target > SEAM:
                _, at_or_above = _classes(score)
                k = int(np.searchsorted(at_or_above, target))
                two_n = target - target % 2
                if at_or_above[k] == target and two_n > (at_or_above[k - 1] if k else 0):
                    yield edge, thr, two_n // 2


def _seam_premise(target=None, at_least=None):
    def check(levels):
        L, = levels
        assert (L["n1"] == target) if target else (L["n1"] >= at_least), L["n1"]
        assert L["n1"] > SEAM or L["n_border"] == L["n1"]                           # up to the seam no select sweeps twice
        assert L["cut2"] is not None and L["n2"] < L["n1"] and abs(2 * L["n2"] - L["n1"]) <= L["n1"] // 8, (L["n1"], L["n2"])   # cuts to roughly half
        if L["n1"] > SEAM:
            assert L["keep2"][SEAM:].any() and not L["keep2"][:SEAM].all()      # the carried offset is used and is not the sweep's size
    return check


def _first_select_premise(levels):
    L, = levels
    assert L["n_border"] > 2 * SEAM and L["cut1"] is not None and L["n1"] < L["n_border"], (L["n_border"], L["n1"])
    assert L["keep1"][2 * SEAM:].any() and L["keep1"][SEAM:2 * SEAM].any() and not L["keep1"][:SEAM].all()
    assert L["class1"] > 1                                                       # FAST scores tie at the cut
    assert L["n1"] > SEAM and L["n2"] < L["n1"]


def cases_a(fast):
    img = block_image(*LARGE)
    out = []
    for target in (SEAM - 1, SEAM, SEAM + 1):
        case, rejected = None, 0                # parameter sets that hand over `target` corners and miss the rest of the premise
        for seed in range(SEED, SEED + 8):      # n1 = 1025 has one corner behind the seam, and it has to be a kept one
            for edge, thr, budget in _seam_search(block_image(LARGE[0], LARGE[1], seed), fast, target):
                case = Case("a_second_select_%d" % target, block_image(LARGE[0], LARGE[1], seed), budget, edge=edge, thr=thr, premise=_seam_premise(target),
                            seed=seed)
                try:
                    case.premise(reference(case, fast)[1])
                    break
                except AssertionError:
                    rejected += 1
            else:
                continue
            break
        case.rejected = rejected                # a search that runs dry leaves its last miss, and the premise fails in the test
        out.append(case)
    border = reference(Case("a_probe", img, 100000), fast)[1][0]["n_border"]
    out.append(Case("a_second_select_2049_or_more", img, (border + 1) // 2, premise=_seam_premise(at_least=2 * SEAM + 1)))
    out.append(Case("a_first_select_cuts", img, 600, premise=_first_select_premise))
    return out


# b. tie classes across the seam ---------------------------------------------------------------------------------------------------------
def _tie_premise(inside):
    def check(levels):
        L, = levels
        h, keep = L["harris"], L["keep2"]
        assert L["cut1"] is None and len(h) == L["n_border"]                     # the first select passes everything on
        assert len(np.unique(h)) >= 20
        assert L["cut2"] is not None and L["n2"] < L["n1"]
        members = h == L["cut2"]
        assert L["class2"] == members.sum() >= 2 and members[:SEAM].any() and members[SEAM:].any()
        above = int((h > L["cut2"]).sum())
        assert L["n2"] == above + L["class2"] and keep[members].all()
        if inside:
            assert above < L["quota"] < L["n2"], (above, L["quota"], L["n2"])    # the cut falls strictly inside the class
        else:
            assert L["n2"] == L["quota"]                                         # the budget ends on the class boundary
    return check


def cases_b(fast):
    img = periodic_image()
    h = reference(Case("b_probe", img, 100000), fast)[1][0]["harris"]
    _, at_or_above = _classes(h)
    half = (len(h) + 1) // 2                                                     # from here on 2 * budget spares the first select
    k = int(np.searchsorted(at_or_above, half))                                  # the median class
    while not max(half, at_or_above[k - 1] + 1) < at_or_above[k]:
        k += 1
    return [Case("b_cut_inside_the_median_class", img, max(half, at_or_above[k - 1] + 1), premise=_tie_premise(True)),
            Case("b_cut_on_a_class_boundary", img, at_or_above[k], premise=_tie_premise(False))]


# c. cut on a negative response ----------------------------------------------------------------------------------------------------------
def _negative_premise(levels):
    L, = levels
    h, keep = L["harris"], L["keep2"]
    assert L["cut1"] is None and L["cut2"] is not None and L["cut2"] < 0
    assert (h[keep] < 0).any() and (h[~keep] < 0).any()


def _positive_premise(levels):
    L, = levels
    h, keep = L["harris"], L["keep2"]
    assert L["cut1"] is None and L["cut2"] is not None and L["cut2"] > 0 and L["cut2"] == h[h > 0].min()
    assert (h < 0).any() and not (h[keep] <= 0).any() and L["n2"] < L["n1"]


def cases_c(fast):
    rejected = 0
    for seed in range(SEED, SEED + 20):
        img = block_image(LARGE[0], LARGE[1], seed)
        h = reference(Case("c_probe", img, 100000), fast)[1][0]["harris"]
        negative = np.unique(h[h < 0])
        if len(negative) >= 2:
            break
        rejected += 1
    cut = negative[len(negative) // 2]                 # ascending: at least one negative response below the cut, the cut itself is kept
    behind = int((h >= cut).sum())
    return [Case("c_cut_on_a_negative_response", img, behind, premise=_negative_premise, rejected=rejected, seed=seed),
            Case("c_cut_on_the_smallest_positive_response", img, int((h > 0).sum()), premise=_positive_premise, rejected=rejected, seed=seed)]


# d. patch and border ------------------------------------------------------------------------------------------------------------------
PATCH_EDGE = [(7, 4), (15, 8), (31, 16), (31, 32), (49, 25), (63, 32)]


def _two_levels_premise(levels):
    assert sum(1 for L in levels if L["n2"] > 0) >= 2


def _some_keypoint_premise(levels):
    L, = levels
    assert (L["rows"], L["cols"]) == (16, 16) and L["n2"] >= 1


def cases_d(fast):
    out = []
    for patch, edge in PATCH_EDGE:
        out.append(Case("d_patch_%d_edge_%d_small" % (patch, edge), block_image(*SMALL), 300, nlevels=3, edge=edge, patch=patch))
        out.append(Case("d_patch_%d_edge_%d_large" % (patch, edge), block_image(*LARGE), 1500, nlevels=3, edge=edge, patch=patch, premise=_two_levels_premise))
    rejected = 0
    for seed in range(SEED, SEED + 50):          # the smallest image the entry takes: one that has a keypoint, so that its angle is compared
        tiny = Case("d_patch_7_edge_4_smallest", block_image(16, 16, seed), 300, nlevels=3, edge=4, patch=7, premise=_some_keypoint_premise, seed=seed)
        if len(reference(tiny, fast)[0]):
            break
        rejected += 1
    tiny.rejected = rejected
    return out + [tiny]


# e. pyramid ---------------------------------------------------------------------------------------------------------------------------
def _top_premise(top, top_rows=None, declared=None):
    def check(levels):
        assert levels[-1]["level"] == top and [L["level"] for L in levels] == list(range(top + 1))
        assert top_rows is None or levels[-1]["rows"] == top_rows
        assert declared is None or len(levels) < declared                        # more levels declared than fit
    return check


def _no_cut_premise(levels):
    assert len(levels) > 1 and all(L["cut1"] is None and L["cut2"] is None and L["n2"] == L["n_border"] > 0 for L in levels)


def _small_budget_premise(budget):
    def check(levels):
        assert len(levels) == 7                 # the declared eighth level, which takes what the rounding left, does not fit
        assert all(L["n2"] >= min(L["quota"], L["n1"]) and (L["quota"] > 0 or L["n2"] == 0) for L in levels)
        assert budget < 7 or all(L["cut2"] is not None and L["n2"] >= 1 for L in levels)
    return check


def cases_e(fast):
    img = block_image(*LARGE)
    out = [Case("e_factor_1.5", img, 1500, scale_factor=1.5, nlevels=8, premise=_top_premise(3, declared=8)),
           Case("e_factor_2.0", img, 1500, scale_factor=2.0, nlevels=8, premise=_top_premise(1, declared=8)),
           Case("e_factor_1.05_levels_16", img, 1500, scale_factor=1.05, nlevels=16, premise=_top_premise(15)),
           Case("e_levels_1", img, 1500, nlevels=1, premise=_top_premise(0)),
           Case("e_levels_2", img, 1500, nlevels=2, premise=_top_premise(1)),
           Case("e_levels_8_budget_1500", img, 1500, nlevels=8, premise=_top_premise(6, declared=8)),
           Case("e_levels_16", img, 1500, nlevels=16, premise=_top_premise(6, declared=16))]
    for rows, top, top_rows in ((83, 0, 83), (84, 1, 70), (85, 1, 71)):         # 84 rows: level 1 has exactly 2 * edge + 8 rows
        out.append(Case("e_rows_%d" % rows, block_image(rows, 120), 200, nlevels=4, premise=_top_premise(top, top_rows, declared=4)))
    for budget in (0, 1, 2, 7, 60):
        out.append(Case("e_budget_%d" % budget, img, budget, nlevels=8, premise=_small_budget_premise(budget)))
    out.append(Case("e_budget_100000", img, 100000, nlevels=8, premise=_no_cut_premise))
    return out


# f. strided rows ----------------------------------------------------------------------------------------------------------------------
def cases_f(fast):
    out = []
    for base in (family("a", fast)[2], family("e", fast)[0]):
        out.append(Case("f_strided_" + base.name, base.img, base.nfeatures, base.scale_factor, base.nlevels, base.edge, base.patch, base.thr,
                        strided=True, premise=base.premise, rejected=base.rejected, seed=base.seed))
    return out


# g. fully independent -----------------------------------------------------------------------------------------------------------------
def _binds_on_two_levels_premise(levels):
    assert len(levels) == 2
    for L in levels:
        assert L["cut1"] is not None and L["n1"] < L["n_border"] and L["cut2"] is not None and 0 < L["n2"] < L["n1"], describe(levels)


def cases_g(fast):
    return [Case("g_python_fast_%dx%d" % shape, block_image(*shape), 24, nlevels=2, python_fast=True, premise=_binds_on_two_levels_premise)
            for shape in ((97, 129), SMALL)]


FAMILIES = {"a": cases_a, "b": cases_b, "c": cases_c, "d": cases_d, "e": cases_e, "f": cases_f, "g": cases_g}
_cases = {}


def family(name, fast):
    """the cases of one family, built once per `fast`"""
    if (name, fast) not in _cases:
        _cases[(name, fast)] = FAMILIES[name](fast)
        assert all(c.family == name for c in _cases[(name, fast)])
    return _cases[(name, fast)]


def all_cases(fast):
    return [c for name in sorted(FAMILIES) for c in family(name, fast)]

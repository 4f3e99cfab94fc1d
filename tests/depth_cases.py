"""What the RGB-D space-map and compute tests share (test_oracle_depth_map.py on the CPU, test_hip_depth_map.py and
test_rgbd_depth_forms_gpu.py on the GPU): adversarial depth images, the cameras, a classifier that counts FROM THE INPUTS which
branches of the z-buffer a case reaches, and thin wrappers over the two entries that expose the row stride and the capacity.

The serial z-buffer and the compute restatement themselves stay where the fixtures are made (tests/golden/make_golden.py:
depth_space_map_ref, depth_compute_ref, _c_round) and are imported, not copied: they associate every sum as the reference does,
(a*x + b*y) + c*z, which a matrix product does not.

The z-buffer's test compares the STORED FLOAT with the new DOUBLE depth.  Per destination, with F0 = float(maximum depth):
the stored float only falls; the first source that brings it to its final value Fmin always passes; from then on only sources
whose float equals Fmin and whose double lies strictly below it (they round UP) still pass.  So several sources of EQUAL raw
depth on one destination end with the last of them (they round up) or the first (they round down), and a source whose float
equals F0 wins only if it rounds up.  `classify` restates exactly that and nothing of the kernels."""
import ctypes as C
import functools

import numpy as np

from golden import make_golden as mg
from vslam_pose_estimation_framework_amd.capi import DepthParams, _p

depth_space_map_ref = mg.depth_space_map_ref
depth_compute_ref = mg.depth_compute_ref
c_round = mg._c_round

SCALE = 1e-3
LEVELS = (0, 1000, 1001, 1003, 1007, 2500, 3299, 3300, 3301, 4000)     # raw values of the tie images
MAX_UP, MAX_DOWN, MAX_FAR = 3.301, 3.3, 10.0                            # float(3.301) > 3.301, float(3.3) < 3.3, no edge
MAXIMA = (MAX_UP, MAX_DOWN, MAX_FAR)
PYTHON_MAX_PIXELS = 120000                                               # the serial Python loop: ~25 us a pixel

COLS = (1, 255, 256, 257, 300, 513)                                      # every 256-column block edge
ROWS = (1, 2, 5, 9, 37)
SHAPES = [(r, c) for r in ROWS for c in COLS]
EXTREMES = [(3, 32767), (32767, 3)]                                      # the int16 maps' last value, the r * cols + c range
PREMISE_SHAPES = [(9, 257), (37, 300), (37, 513)]                        # large enough for the tie counts below
MIN_TIES, MIN_EDGE = 100, 20
OFFSET_SHAPES = [(9, 257), (37, 300), (48, 64)]


def params(rows, cols, Kl, Kr, r2l, maximum_depth, minimum_depth=0.1, tri=1, binning=1, bin_px=6, scale=SCALE):
    return DepthParams.make(rows, cols, Kl, np.linalg.inv(Kl), np.linalg.inv(Kr), r2l, scale, minimum_depth, maximum_depth, tri, binning, bin_px)


def with_compute(p, minimum_depth, maximum_depth, tri, binning, bin_px):
    q = DepthParams.from_buffer_copy(p)
    q.minimum_depth_meters, q.maximum_depth_meters = minimum_depth, maximum_depth
    q.enable_point_triangulation, q.enable_keypoint_binning, q.bin_size_pixels = int(tri), int(binning), int(bin_px)
    return q


# ---- cases ---------------------------------------------------------------------------------------------------------------------
def shrinking_camera(rows, cols):
    """K_right with focal f, K_left with f / 2, one principal point, no offset: u' = (u + cx) / 2, about four sources a destination."""
    f = 0.9 * max(rows, cols) + 3.0
    cx, cy = (cols - 1) / 2.0, (rows - 1) / 2.0
    Kr = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1.0]])
    Kl = np.array([[f / 2, 0, cx], [0, f / 2, cy], [0, 0, 1.0]])
    return Kl, Kr, np.eye(4)[:3].copy()


@functools.lru_cache(maxsize=None)
def tie_case(rows, cols, seed, maximum_depth):
    """(depth, p): 5 x 5 blocks of equal raw depth drawn from LEVELS under the shrinking camera."""
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, len(LEVELS), ((rows + 4) // 5, (cols + 4) // 5))
    depth = np.asarray(LEVELS, np.uint16)[np.kron(blocks, np.ones((5, 5), np.int64))[:rows, :cols]]
    depth = np.ascontiguousarray(depth)
    depth.setflags(write=False)
    Kl, Kr, r2l = shrinking_camera(rows, cols)
    return depth, params(rows, cols, Kl, Kr, r2l, maximum_depth)


@functools.lru_cache(maxsize=None)
def offset_case(rows, cols, seed, maximum_depth=10.0, behind=6):
    """(depth, p): a depth camera rotated by 0.01 rad and shifted by (0.025, 0, -0.35) m against the colour camera, with another
    matrix (test_rgbd_components_at_sensor_size_against_oracle's, scaled to the image); random depths of 0.5 .. 8 m with holes,
    and `behind` sources of 0.2 .. 0.34 m that the negative t_z puts behind the left camera."""
    rng = np.random.default_rng(seed)
    f = 525.0 * cols / 640.0
    Kr = np.array([[f, 0, (cols - 1) / 2.0], [0, f, (rows - 1) / 2.0], [0, 0, 1.0]])
    Kl = np.array([[f * 0.98, 0, (cols - 1) / 2.0 + 1.5], [0, f * 0.98, (rows - 1) / 2.0 - 2.0], [0, 0, 1.0]])
    ang = 0.01
    r2l = np.hstack([np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]), np.array([[0.025], [0.0], [-0.35]])])
    depth = rng.integers(500, 8000, (rows, cols)).astype(np.uint16)
    depth[rng.random((rows, cols)) < 0.1] = 0
    flat = rng.choice(rows * cols, behind, replace=False)
    depth.reshape(-1)[flat] = rng.integers(200, 340, behind).astype(np.uint16)
    depth.setflags(write=False)
    return depth, params(rows, cols, Kl, Kr, r2l, maximum_depth, bin_px=10)


# ---- the classifier -------------------------------------------------------------------------------------------------------------
def _mat(a):
    return np.array(list(a), np.float64)


def project(depth, p):
    """Every pixel's projection with the reference's association, elementwise in float64 (numpy neither fuses nor reorders
    elementwise products and sums): dict of flat arrays in scan order."""
    rows, cols = depth.shape
    Ki, T, K = _mat(p.K_right_inverse), _mat(p.right_to_left), _mat(p.K_left)
    r, c = np.mgrid[0:rows, 0:cols]
    r, c = r.ravel().astype(np.float64), c.ravel().astype(np.float64)
    raw = depth.ravel().astype(np.int64)
    dm = raw * p.depth_scale_factor_intensity_to_meters
    ph = (c * dm, r * dm, dm)
    pr = [(Ki[3 * i] * ph[0] + Ki[3 * i + 1] * ph[1]) + Ki[3 * i + 2] * ph[2] for i in range(3)]
    pl = [((T[4 * i] * pr[0] + T[4 * i + 1] * pr[1]) + T[4 * i + 2] * pr[2]) + T[4 * i + 3] for i in range(3)]
    px = [(K[3 * i] * pl[0] + K[3 * i + 1] * pl[1]) + K[3 * i + 2] * pl[2] for i in range(3)]
    valid = raw != 0
    front = valid & (pl[2] > 0)
    with np.errstate(all="ignore"):
        u = np.where(front, px[0] / np.where(front, px[2], 1.0), 0.0)
        v = np.where(front, px[1] / np.where(front, px[2], 1.0), 0.0)

    def c_round(x):                               # std::round: half away from zero (x - trunc(x) is exact)
        t = np.trunc(x)
        return t + np.sign(x) * (np.abs(x - t) >= 0.5)
    ru, rv = c_round(u), c_round(v)
    return dict(valid=valid, front=front, behind=valid & ~front, z=pl[2], pl=pl, u=u, v=v, ru=ru, rv=rv,
                inside=front & (rv >= 0) & (rv < rows) & (ru >= 0) & (ru < cols))


def classify(depth, p):
    """Counts of what the z-buffer meets on (depth, p), and the winner it must end with, per destination, from the rule in this
    file's header.  Keys: multi, tie_first, tie_later, edge_won, edge_lost, outside (left, right, top, bottom), behind, filled,
    moved, max_abs_uv; winner: flat source index per destination or -1."""
    rows, cols = depth.shape
    n = rows * cols
    q = project(depth, p)
    F0 = np.float32(p.maximum_depth_meters)
    src = np.nonzero(q["inside"])[0]
    dest = (q["rv"][src] * cols + q["ru"][src]).astype(np.int64)
    order = np.argsort(dest, kind="stable")                   # scan order survives inside a destination
    src, dest = src[order], dest[order]
    z = q["z"][src]
    zf = z.astype(np.float32)
    winner = -np.ones(n, np.int64)
    out = dict(multi=0, tie_first=0, tie_later=0, edge_won=0, edge_lost=0)
    if len(src):
        starts = np.nonzero(np.r_[True, dest[1:] != dest[:-1]])[0]
        counts = np.diff(np.r_[starts, len(dest)])
        gid = np.repeat(np.arange(len(starts)), counts)
        fmin = np.minimum(np.minimum.reduceat(zf, starts), F0)
        in_s = zf == fmin[gid]
        up = in_s & (z < fmin[gid].astype(np.float64))
        first = np.minimum.reduceat(np.where(in_s, src, n), starts)
        last_up = np.maximum.reduceat(np.where(up, src, -1), starts)
        n_s = np.add.reduceat(in_s.astype(np.int64), starts)
        below = fmin < F0
        win = np.where(below, np.maximum(first, last_up), last_up)       # first < every other member of S
        win = np.where(~below & (n_s == 0), -1, win)
        winner[dest[starts]] = win
        out["multi"] = int((counts >= 2).sum())
        out["tie_first"] = int((below & (n_s >= 2) & (win == first)).sum())
        out["tie_later"] = int((below & (n_s >= 2) & (win != first)).sum())
        out["edge_won"] = int((~below & (n_s >= 1) & (win >= 0)).sum())
        out["edge_lost"] = int((~below & (n_s >= 1) & (win < 0)).sum())
    f = q["front"]
    out["outside"] = (int((f & (q["ru"] < 0)).sum()), int((f & (q["ru"] >= cols)).sum()), int((f & (q["rv"] < 0)).sum()), int((f & (q["rv"] >= rows)).sum()))
    out["behind"] = int(q["behind"].sum())
    out["filled"] = int((winner >= 0).sum())
    out["moved"] = int(((winner >= 0) & (winner != np.arange(n))).sum())
    out["max_abs_uv"] = float(max(np.abs(q["u"]).max(), np.abs(q["v"]).max())) if n else 0.0
    out["winner"] = winner
    return out


def maps_of(winner, rows, cols):
    """(row_map, col_map) a winner array stands for."""
    w = winner.reshape(rows, cols)
    return np.where(w >= 0, w // cols, -1).astype(np.int16), np.where(w >= 0, w % cols, -1).astype(np.int16)


def rounding_of_the_maxima():
    """The premise of MAX_UP / MAX_DOWN."""
    return float(np.float32(MAX_UP)) > MAX_UP and float(np.float32(MAX_DOWN)) < MAX_DOWN


def assert_tie_premises(cl, maximum_depth, tag):
    assert cl["max_abs_uv"] < 2.0 ** 31, tag
    assert cl["tie_first"] >= MIN_TIES and cl["tie_later"] >= MIN_TIES, (tag, cl["tie_first"], cl["tie_later"])
    if maximum_depth == MAX_UP:
        assert cl["edge_won"] >= MIN_EDGE and cl["edge_lost"] == 0, (tag, cl["edge_won"], cl["edge_lost"])
    if maximum_depth == MAX_DOWN:
        assert cl["edge_lost"] >= MIN_EDGE and cl["edge_won"] == 0, (tag, cl["edge_won"], cl["edge_lost"])


def assert_offset_premises(cl, tag):
    assert cl["max_abs_uv"] < 2.0 ** 31, tag
    assert cl["behind"] >= 1 and min(cl["outside"]) >= 1, (tag, cl["behind"], cl["outside"])
    assert cl["moved"] >= 0.3 * cl["filled"] > 0, (tag, cl["moved"], cl["filled"])


# ---- the entries with their row stride and capacity in the open ------------------------------------------------------------------
def space_map(api, p, depth, stride=None):
    """api.depth_space_map with the depth rows `stride` elements apart (depth: 2-D array at least p.cols wide).  Returns
    (rc, space, row_map, col_map); the outputs are pre-filled so that an entry that writes nothing shows."""
    depth = np.ascontiguousarray(depth, np.uint16)
    rows, cols = int(p.rows), int(p.cols)
    space = np.full((rows, cols, 3), -7.0, np.float32)
    rmap = np.full((rows, cols), -7, np.int16); cmap = np.full((rows, cols), -7, np.int16)
    rc = api.fn("depth_space_map")(*api._ctx_args(), C.byref(p), _p(depth, C.c_uint16), C.c_int32(depth.shape[1] if stride is None else stride),
                                   _p(space, C.c_float), _p(rmap, C.c_int16), _p(cmap, C.c_int16))
    return rc, space, rmap, cmap


def compute(api, p, space, rc_features, rc_tracked, cap):
    """api.depth_compute with the status and the counts returned instead of raised: (rc, n_new, n_temp, new, xyz, temp, temp_xyz),
    the lists cut to min(count, cap)."""
    rcf = np.ascontiguousarray(rc_features, np.int32).reshape(-1, 2)
    rct = np.ascontiguousarray(rc_tracked, np.int32).reshape(-1, 2)
    sp = None if space is None else np.ascontiguousarray(space, np.float32)
    room = max(cap, 1)
    nf, xyz = np.full(room, -9, np.int32), np.zeros((room, 3), np.float64)
    tf_, txyz = np.full(room, -9, np.int32), np.zeros((room, 3), np.float64)
    nn, nt = C.c_int32(-1), C.c_int32(-1)
    rc = api.fn("depth_compute")(*api._ctx_args(), C.byref(p), None if sp is None else _p(sp, C.c_float), C.c_int32(rcf.shape[0]), _p(rcf, C.c_int32),
                                 C.c_int32(rct.shape[0]), _p(rct, C.c_int32), C.c_int32(cap), C.byref(nn), _p(nf, C.c_int32), _p(xyz, C.c_double),
                                 C.byref(nt), _p(tf_, C.c_int32), _p(txyz, C.c_double))
    a, b = min(max(nn.value, 0), cap), min(max(nt.value, 0), cap)
    return rc, nn.value, nt.value, nf[:a].copy(), xyz[:a].copy(), tf_[:b].copy(), txyz[:b].copy()


# ---- compute cases ---------------------------------------------------------------------------------------------------------------
BIN = 8                                  # even (half-way borders exist) and divides neither 75 nor 601
NF = (0, 1, 1023, 1024, 1025, 3000)      # both sides of the 1024-thread chunk
NT = (0, 1, 700)
COMPUTE_SHAPE = (75, 601)          # the shrinking camera fills its central quarter: 38 x 300 pixels, 5 x 38 bins
# (minimum, maximum) of the compute parameters: the tie map's own edge maxima, and limits that ARE depths of the map
# (1000 * 1e-3 == 1.0 and 4000 * 1e-3 rounds to float 4.0 exactly): "not below the minimum" keeps, "at the maximum" is temporary
LIMITS = ((0.1, MAX_UP), (1.0, 4.0))


@functools.lru_cache(maxsize=None)
def compute_features(seed=3):
    """3000 features and 700 tracked points on the 75 x 601 tie map: (features [3000][2], tracked [700][2]).  The first features
    are the special ones, so that every prefix of 1023 and more holds them: the four corners, one pixel twice, pixels whose row or
    column is an odd multiple of BIN / 2; the rest are random pixels, four in five of them inside the filled quarter, repeats allowed
    (a feature list may hold a pixel twice)."""
    rows, cols = COMPUTE_SHAPE
    rng = np.random.default_rng(seed)
    special = [(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1), (37, 301), (37, 301)]
    half = BIN // 2
    special += [(half * (2 * i + 1), int(c)) for i in range(rows // BIN) for c in rng.integers(0, cols, 6)]
    special += [(int(r), half * (2 * j + 1)) for j in range(0, cols // BIN, 2) for r in rng.integers(0, rows, 2)]
    special += [(half * (2 * i + 1), half * (2 * j + 1)) for i in range(rows // BIN) for j in range(0, cols // BIN, 5)]
    def pixels(n):
        inner = rng.random(n) < 0.8
        r = np.where(inner, rng.integers(rows // 4, 3 * rows // 4, n), rng.integers(0, rows, n))
        c = np.where(inner, rng.integers(cols // 4, 3 * cols // 4, n), rng.integers(0, cols, n))
        return np.stack([r, c], axis=1).astype(np.int32)
    feats = np.vstack([np.array(special, np.int32), pixels(3000 - len(special))])
    tracked = pixels(700)
    feats.setflags(write=False); tracked.setflags(write=False)
    return feats, tracked


def bin_of(row, col, bin_px):
    return (round(row / bin_px), round(col / bin_px))          # Python's round: half to even, as rint


def compute_premises(space, feats, tracked, minimum, maximum, tri, bin_px):
    """Counted from the inputs: bins whose minimum depth is shared by >= 2 candidates, features on a half-way bin border, tracked
    points in bins that also hold candidates, features on a depth equal to the minimum / the maximum, pixels held twice."""
    z = space[feats[:, 0], feats[:, 1], 2].astype(np.float64) if len(feats) else np.zeros(0)
    cand = (z >= minimum) & ~((z >= maximum) & bool(tri))
    per_bin = {}
    for i in np.nonzero(cand)[0]:
        per_bin.setdefault(bin_of(int(feats[i, 0]), int(feats[i, 1]), bin_px), []).append(z[i])
    shared = sum(1 for v in per_bin.values() if sum(1 for x in v if x == min(v)) >= 2)
    halfway = int(((feats[:, 0] % bin_px == bin_px // 2) | (feats[:, 1] % bin_px == bin_px // 2)).sum()) if bin_px % 2 == 0 and len(feats) else 0
    tbins = set(bin_of(int(r), int(c), bin_px) for r, c in tracked)
    pixels = feats[:, 0].astype(np.int64) * 100000 + feats[:, 1] if len(feats) else np.zeros(0, np.int64)
    return dict(shared_minimum_bins=shared, halfway=halfway, tracked_bins_with_candidates=len(tbins & set(per_bin)),
                at_minimum=int((z == minimum).sum()), at_maximum=int((z == maximum).sum()), repeated_pixels=int(len(pixels) - len(np.unique(pixels))))


def compute_ref(space, feats, tracked, p):
    """depth_compute_ref on a DepthParams: (new, xyz, temp, temp_xyz) as the entries return them."""
    Kli = _mat(p.K_left_inverse).reshape(3, 3)
    new, temp = depth_compute_ref(space, [(int(r), int(c)) for r, c in feats], [(int(r), int(c)) for r, c in tracked], Kli, p.minimum_depth_meters,
                                  p.maximum_depth_meters, bool(p.enable_point_triangulation), bool(p.enable_keypoint_binning), p.bin_size_pixels)
    xyz = np.array([space[feats[i, 0], feats[i, 1]] for i in new], np.float64).reshape(-1, 3)
    return (np.array(new, np.int32), xyz, np.array([i for i, _ in temp], np.int32), np.array([x for _, x in temp], np.float64).reshape(-1, 3))


# ---- comparisons: `api` is the implementation under test, `orc` the oracle (the CPU twin passes the oracle as `api` and None here) ----
_solved = {}


def solved(orc, kind, rows, cols, seed, maximum):
    """One case worked out once per process and shared by every test that needs it: dict of depth, p, cl (classify), oracle
    (space, row_map, col_map) and python (the serial restatement's three, or None above PYTHON_MAX_PIXELS)."""
    key = (kind, rows, cols, seed, maximum)
    if key not in _solved:
        depth, p = (tie_case if kind == "tie" else offset_case)(rows, cols, seed, maximum)
        rc, space, rmap, cmap = space_map(orc, p, depth)
        assert rc == 0, key
        python = None
        if rows * cols <= PYTHON_MAX_PIXELS:
            python = depth_space_map_ref(depth, _mat(p.K_left).reshape(3, 3), _mat(p.K_right_inverse).reshape(3, 3), _mat(p.right_to_left).reshape(3, 4),
                                         p.depth_scale_factor_intensity_to_meters, p.maximum_depth_meters)
        for a in (space, rmap, cmap) + (python or ()):
            a.setflags(write=False)
        _solved[key] = dict(depth=depth, p=p, cl=classify(depth, p), oracle=(space, rmap, cmap), python=python)
    return _solved[key]


def same_maps(got, want, tag):
    np.testing.assert_array_equal(got[0].view(np.uint32), want[0].view(np.uint32), err_msg="%s space" % (tag,))
    np.testing.assert_array_equal(got[1], want[1], err_msg="%s row_map" % (tag,))
    np.testing.assert_array_equal(got[2], want[2], err_msg="%s col_map" % (tag,))


def check_oracle_side(s, tag):
    """Oracle == restatement (where it was run) == the winners `classify` predicts; space holds the winner's float coordinates."""
    rows, cols = s["depth"].shape
    if s["python"] is not None:
        same_maps(s["oracle"], s["python"], "%s oracle against python" % (tag,))
    wr, wc = maps_of(s["cl"]["winner"], rows, cols)
    np.testing.assert_array_equal(s["oracle"][1], wr, err_msg="%s classify rows" % (tag,))
    np.testing.assert_array_equal(s["oracle"][2], wc, err_msg="%s classify cols" % (tag,))
    empty = s["cl"]["winner"].reshape(rows, cols) < 0
    assert np.all(s["oracle"][0][empty] == np.array([0, 0, np.float32(s["p"].maximum_depth_meters)], np.float32)), tag


def check_against(api, s, tag, sentinel=None):
    """api == oracle (== restatement) on the solved case, bit for bit; with `sentinel`, once more on rows padded by seven elements
    of that value, which must never be read as depth."""
    rc, space, rmap, cmap = space_map(api, s["p"], s["depth"])
    assert rc == 0, tag
    same_maps((space, rmap, cmap), s["oracle"], tag)
    if s["python"] is not None:
        same_maps((space, rmap, cmap), s["python"], "%s against python" % (tag,))
    if sentinel is not None:
        rows, cols = s["depth"].shape
        padded = np.full((rows, cols + 7), sentinel, np.uint16)
        padded[:, :cols] = s["depth"]
        rc, space, rmap, cmap = space_map(api, s["p"], padded)
        assert rc == 0, tag
        same_maps((space, rmap, cmap), s["oracle"], "%s padded rows" % (tag,))


def compute_sweep(api, orc, space, p, binning, tri, resident=False):
    """vslam_depth_compute over NF x NT x LIMITS x bin sizes against the oracle (when given) and depth_compute_ref: lists, order and
    coordinates exact; cap == the larger list passes, one below returns VSLAM_ERR_CAPACITY with the true counts.  resident: the map
    the last space-map call left in the context (space = None in the call).  Returns the premise counts of the largest case."""
    feats, tracked = compute_features()
    worst = None
    n_calls = 0
    for minimum, maximum in LIMITS:
        for bin_px in ((BIN, 3) if binning else (BIN,)):
            q = with_compute(p, minimum, maximum, tri, binning, bin_px)
            for nF in NF:
                for nT in NT:
                    tag = (minimum, maximum, bin_px, nF, nT, binning, tri)
                    f, t = feats[:nF], tracked[:nT]
                    want = compute_ref(space, f, t, q)
                    cap = max(len(want[0]), len(want[2]))
                    got = compute(api, q, None if resident else space, f, t, cap)
                    assert got[:3] == (0, len(want[0]), len(want[2])), (tag, got[:3], len(want[0]), len(want[2]))
                    for a, b in zip(got[3:], want):
                        np.testing.assert_array_equal(a, b, err_msg=str(tag))
                    if orc is not None:
                        ref = compute(orc, q, space, f, t, cap)
                        assert ref[:3] == got[:3], tag
                        for a, b in zip(got[3:], ref[3:]):
                            np.testing.assert_array_equal(a, b, err_msg=str(tag))
                    if cap > 0:
                        low = compute(api, q, None if resident else space, f, t, cap - 1)
                        assert low[:3] == (-4, len(want[0]), len(want[2])), (tag, low[:3])
                    n_calls += 1
                    if nF == NF[-1] and nT == NT[-1] and bin_px == BIN:
                        worst = compute_premises(space, f, t, minimum, maximum, tri, bin_px)
                        worst["n_new"], worst["n_temp"] = len(want[0]), len(want[2])
                        if binning:
                            assert worst["shared_minimum_bins"] >= 50 and worst["halfway"] >= 100 and worst["tracked_bins_with_candidates"] >= 20, (tag, worst)
                        assert worst["repeated_pixels"] >= 1, (tag, worst)
                        if (minimum, maximum) == LIMITS[1]:
                            assert worst["at_minimum"] >= 10 and worst["at_maximum"] >= 10, (tag, worst)
    return worst, n_calls


# ---- the device-resident loop's launch forms (test_rgbd_depth_forms_host.py, test_rgbd_depth_forms_gpu.py) ----------------------------
LOOP_FRAMES = 10
LOOP_SEEDS = (23, 31, 47)
STRIP_BATCHES = (24, 48)               # streams of the strip-walk cases
DEPTH_UNIT = 2e-3
INFO_FIELDS = (("status", "status"), ("n_keypoints", "n_keypoints_left"), ("n_tracked", "n_tracked"), ("n_lost", "n_lost"),
               ("n_tracked_landmarks", "n_tracked_landmarks"), ("aligner_ran", "aligner_ran"), ("n_inliers", "n_inliers"),
               ("aligner_iterations", "aligner_iterations"), ("n_after_prune", "n_after_prune"), ("n_recovered", "n_recovered"),
               ("n_active_landmarks", "n_active_landmarks"), ("n_new", "n_new_stereo"), ("n_points", "n_points"),
               ("window_pixels", "window_pixels"), ("track_attempts", "track_attempts"), ("fallback", "fallback"),
               ("track_broken", "track_broken"), ("status_at_start", "status_at_start"))
POSE_RTOL = 1e-4


def is_plain(p):
    """kernels_depth.h depth_source / rgbd_device.h create(): pinhole matrices and an identity offset — the one-pass k_depth_direct
    runs first and the general passes wait behind its gate."""
    Ki, K, T = _mat(p.K_right_inverse), _mat(p.K_left), _mat(p.right_to_left)
    return bool(Ki[1] == 0 and Ki[3] == 0 and Ki[6] == 0 and Ki[7] == 0 and Ki[8] == 1 and K[1] == 0 and K[3] == 0 and K[6] == 0 and K[7] == 0 and K[8] == 1 and
                np.array_equal(T, np.eye(4)[:3].ravel()))


def loop_camera(kind, p):
    """The tracker's depth parameters with another depth camera.  offset: focal x 1.02, centre shifted, rotated by 0.01 rad and moved
    by (0.02, 0, 0.001) m (not plain: the ungated general passes).  crossing: focal x 1.25 and no offset (plain: k_depth_direct
    runs, finds its sources on other pixels and opens the gate).  registered: the depth image of the colour camera."""
    q = DepthParams.from_buffer_copy(p)
    if kind == "registered":
        return q
    K = _mat(p.K_left).reshape(3, 3)
    Kr = K.copy()
    if kind == "offset":
        Kr[0, 0] *= 1.02; Kr[1, 1] *= 1.02; Kr[0, 2] += 2.5; Kr[1, 2] -= 1.5
        ang = 0.01
        r2l = np.hstack([np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]), np.array([[0.02], [0.0], [0.001]])])
    else:
        assert kind == "crossing"
        Kr[0, 0] *= 1.25; Kr[1, 1] *= 1.25
        r2l = np.eye(4)[:3]
    q.K_right_inverse[:] = list(np.linalg.inv(Kr).ravel())
    q.right_to_left[:] = list(np.ascontiguousarray(r2l, np.float64).ravel())
    return q


_loops = {}


def checker_run(kind, seed, zero_first=False):
    """The checker loop (tests/rgbd_loop.py over the oracle) on LOOP_FRAMES frames of the tum configuration with `kind`'s depth camera,
    once per process: dict of cfg, p, frames [(image, depth)], info [per frame], points [per frame: arrays], z / src [per frame: the
    oracle's winning depth and flat source index per destination].  The renderer's depth does not depend on the seed, so the second
    and third seed start two and four frames into their scene: no two sequences of a batch share a depth image."""
    key = (kind, seed, zero_first)
    if key in _loops:
        return _loops[key]
    from _oracle import Oracle
    from rgbd_loop import RgbdTracker as PyLoop
    from test_rgbd_mode import setup
    o = Oracle()
    try:
        scene, cfg, p0 = setup(o, "tum", descriptor=1, seed=seed)
        p = loop_camera(kind, p0)
        o.create(cfg, 0, 1)
        ref = PyLoop(o, cfg, p)
        out = dict(cfg=cfg, p=p, frames=[], info=[], points=[], z=[], src=[])
        start = 2 * LOOP_SEEDS.index(seed) if seed in LOOP_SEEDS else 0
        for k in range(LOOP_FRAMES):
            L, D = o.render(scene, start + k)[0], o.render_depth(scene, start + k, DEPTH_UNIT)
            if zero_first and k == 0:
                D = np.zeros_like(D)
            info = dict(ref.process(L, D))
            cur = ref.frames[-1]
            prevlist = (ref.frames[-2].points + ref.frames[-2].temps) if k else []
            index_of = {id(q): i for i, q in enumerate(prevlist)}
            n = len(cur.points)
            pts = dict(xy=np.array([q.xy for q in cur.points], np.float32).reshape(n, 2), desc=np.array([q.desc for q in cur.points], np.uint8).reshape(n, 32),
                       cam=np.array([q.cam for q in cur.points], np.float64).reshape(n, 3),
                       meta=np.array([[index_of[id(q.previous)] if q.previous is not None else -1, q.track_len, q.landmark.updates if q.landmark is not None else 0,
                                       int(q.unreliable)] for q in cur.points], np.int32).reshape(n, 4))
            _, space, rmap, cmap = space_map(o, p, D)
            out["frames"].append((L, D)); out["info"].append(info); out["points"].append(pts)
            out["z"].append(space[:, :, 2].copy()); out["src"].append(np.where(rmap >= 0, rmap.astype(np.int64) * p.cols + cmap, -1))
    finally:
        o.destroy()
    _loops[key] = out
    return out


def loop_premises(run):
    """From the checker loop and the oracle's maps alone."""
    rows, cols = run["z"][0].shape
    own = np.arange(rows * cols).reshape(rows, cols)
    filled = [s >= 0 for s in run["src"]]
    F0 = np.float32(run["p"].maximum_depth_meters)
    grows = [int(((run["z"][k + 1] > run["z"][k]) & filled[k] & (run["z"][k] < F0)).sum()) for k in range(len(run["z"]) - 1)]
    return dict(status=[i["status"] for i in run["info"]], tracked=[i["n_tracked"] for i in run["info"]],
                filled=[int(f.sum()) for f in filled], moved=[int((f & (s != own)).sum()) for f, s in zip(filled, run["src"])], grows=grows)


def assert_loop_premises(pr, tag):
    assert all(s == 1 for s in pr["status"][5:]) and min(pr["tracked"][5:]) >= 50, (tag, pr["status"], pr["tracked"])
    assert all(m >= 0.3 * f > 0 for m, f in zip(pr["moved"], pr["filled"])), (tag, pr["moved"], pr["filled"])
    assert min(pr["grows"]) >= 1000, (tag, pr["grows"])


def info_tuple(fi, nt):
    """Every field of a frame's report, for product-against-product comparisons (bit for bit: the poses are in it)."""
    out = []
    for name, _ in fi._fields_:
        v = getattr(fi, name)
        out.append((name, tuple(v) if hasattr(v, "__len__") else v))
    return tuple(out) + (("n_temporary", nt),)


def assert_same_run(got, want, tag):
    """[(info_tuple, points)] per frame, bit for bit."""
    assert len(got) == len(want), tag
    for f, ((ia, pa), (ib, pb)) in enumerate(zip(got, want)):
        for (name, va), (_, vb) in zip(ia, ib):
            assert va == vb, (tag, f, name, va, vb)
        for key in ("xy", "cam", "meta", "desc"):
            np.testing.assert_array_equal(pa[key], pb[key], err_msg="%s frame %d %s" % (tag, f, key))


def assert_frame_equals_checker(run, k, fi, n_temp, pts, tag):
    """test_rgbd_tracker_matches_the_checker_loop's comparison: counters, thresholds and point lists exact, pose to 1e-4; the camera
    coordinates bit for bit where they come straight from the space map (three floats widened: every measured, tracked and recovered
    point), to that test's 1e-12 where getPointInCamera triangulated them."""
    a, want = run["info"][k], run["points"][k]
    for name, field in INFO_FIELDS:
        assert a[name] == getattr(fi, field), (tag, k, name, a[name], getattr(fi, field))
    assert a["thresholds"] == list(fi.thresholds)[:len(a["thresholds"])] and a["n_temporary"] == n_temp and a["tau_track"] == fi.tau_track, (tag, k)
    To, Tg = a["pose"], np.array(fi.camera_left_to_world).reshape(3, 4)
    assert np.linalg.norm(Tg - To) / np.linalg.norm(To) <= POSE_RTOL, (tag, k)
    assert len(pts["xy"]) == len(want["xy"]), (tag, k)
    np.testing.assert_array_equal(pts["xy"].view(np.uint32), want["xy"].view(np.uint32), err_msg="%s frame %d xy" % (tag, k))
    np.testing.assert_array_equal(pts["desc"], want["desc"], err_msg="%s frame %d desc" % (tag, k))
    np.testing.assert_array_equal(pts["meta"][:, :4], want["meta"], err_msg="%s frame %d meta" % (tag, k))
    from_map = np.all(want["cam"].astype(np.float32).astype(np.float64) == want["cam"], axis=1)
    np.testing.assert_array_equal(pts["cam"][from_map], want["cam"][from_map], err_msg="%s frame %d cam" % (tag, k))
    np.testing.assert_allclose(pts["cam"][~from_map], want["cam"][~from_map], rtol=1e-12, atol=0, err_msg="%s frame %d triangulated cam" % (tag, k))
    return int(from_map.sum())

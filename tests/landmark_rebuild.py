"""Landmark creation / refinement of the fused tracker (`Landmark::Landmark`, `Landmark::update` as PoseTracker3D::_updatePoints
applies them to the points of a frame) restated in float64 numpy from what the C ABI exports after every frame:

    points(s)    meta[:, 2] previous index, meta[:, 3] track length, meta[:, 4] landmark updates; cam; lm
    poses(s, f)  camera to world of the frame (world to camera: its numpy inverse)

Per stream the rebuild keeps the point lists and poses of the last `ring` frames (`max_history_frames`: what the tracker itself can
still address).  For every point of the new frame whose track is long enough it rebuilds the measurement list, newest first, by
following `prev` through its own stored frames, cut to min(track length + 1, ring) entries, and either creates the landmark (the mean
of the measurements' world coordinates) or refines the estimate the point carries: its predecessor's exported `lm` and update count —
a tracked or recovered point takes both over from the point it continues.

Nothing here follows the kernels' order of accumulation: sums over a list run in list order or through numpy, the 3 x 3 systems
go to numpy.linalg.solve.  Every discrete decision of an update (convergence test, saturated kernel, point behind the camera,
accept / reset / keep) records how far it was from its threshold; an update with a margin below MARGIN cannot be judged by
a float comparison and is reported as undecidable instead.

Test infrastructure only (a plain module, no fixtures)."""
import collections

import numpy as np

MARGIN = 1e-9            # smallest relative distance from a threshold at which a decision still counts as decided
CONVERGENCE = 1e-5       # Landmark::update stops when the total error changes by less than this
CREATE, ACCEPT, RESET, KEEP, UNFINISHED = 0, 1, 2, 3, 4    # what happened to the landmark of a point
KIND_NAMES = ("create", "accept", "reset", "keep", "unfinished")

FrameResult = collections.namedtuple(
    "FrameResult", "index kind n_meas length lm lmup margin carried carried_lmup truncated iterations")
FrameResult.__doc__ = """One frame of one stream.  index: the eligible points; kind: CREATE .. UNFINISHED; n_meas: track length + 1;
length: measurements used (n_meas cut to the ring); lm, lmup: expected landmark and update count; margin: smallest decision margin
(inf for creations); carried, carried_lmup: the predecessor's estimate; truncated: n_meas > ring; iterations: Gauss-Newton rounds."""


def _apply(T, p):
    """Rigid transform of points: T [..., 3, 4], p [..., 3]."""
    return ((T[..., 0] * p[..., None, 0] + T[..., 1] * p[..., None, 1]) + T[..., 2] * p[..., None, 2]) + T[..., 3]


def _rel(a, threshold):
    return np.abs(a - threshold) / abs(threshold)


class LandmarkRebuild(object):
    """One stream.  frame(points, camera_to_world) consumes the export of the next frame and returns its FrameResult."""

    def __init__(self, cfg, ring=None):
        self.ring = int(cfg.max_history_frames if ring is None else ring)
        self.min_track = int(cfg.minimum_track_length_for_landmark_creation)
        self.kernel = float(cfg.landmark_maximum_error_squared_meters)
        self.max_iterations = int(cfg.landmark_maximum_number_of_iterations)
        self.history = collections.deque(maxlen=self.ring)      # newest last: (prev, cam, camera_to_world, world_to_camera)
        self.previous = None                                    # (lm, lmup) of the previous frame's export

    def reset(self):
        self.history.clear()
        self.previous = None

    # -- measurement lists ---------------------------------------------------------------------------------------
    def _lists(self, index, length):
        """idx [n, L] point index of measurement k in frame f - k (-1 beyond the list), newest first; valid [n, L]."""
        L = len(self.history)
        idx = np.full((len(index), L), -1, np.int64)
        idx[:, 0] = index
        for k in range(1, L):
            prev = self.history[-k][0]                           # links of frame f - (k - 1)
            cur = idx[:, k - 1]
            go = (cur >= 0) & (k < length)
            nxt = np.full(len(index), -1, np.int64)
            nxt[go] = prev[cur[go]]
            idx[:, k] = nxt                                      # a negative link ends the list
        return idx, idx >= 0

    def frame(self, points, camera_to_world):
        meta = np.asarray(points["meta"])
        cam = np.asarray(points["cam"], np.float64)
        c2w = np.asarray(camera_to_world, np.float64).reshape(3, 4)
        w2c = np.linalg.inv(np.vstack([c2w, [0.0, 0.0, 0.0, 1.0]]))[:3]
        self.history.append((meta[:, 2].astype(np.int64), cam.copy(), c2w, w2c))
        L = len(self.history)
        tlen = meta[:, 3].astype(np.int64)
        index = np.nonzero(tlen >= self.min_track)[0]
        n = len(index)
        n_meas = tlen[index] + 1
        length = np.minimum(n_meas, self.ring)
        assert n == 0 or length.max() <= L, "a track is longer than the frames seen so far"
        truncated = n_meas > self.ring
        prev_index = meta[index, 2]
        carried = np.zeros((n, 3))
        carried_lmup = np.zeros(n, np.int64)
        if self.previous is not None:
            has = prev_index >= 0
            carried[has] = self.previous[0][prev_index[has]]
            carried_lmup[has] = self.previous[1][prev_index[has]]
        idx, valid = self._lists(index, length)
        # measurements and frames of the lists: frame f - k is history[-1 - k]
        M = np.zeros((n, L, 3))
        for k in range(L):
            rows = valid[:, k]
            M[rows, k] = self.history[-1 - k][1][idx[rows, k]]
        C2W = np.stack([self.history[-1 - k][2] for k in range(L)])
        W2C = np.stack([self.history[-1 - k][3] for k in range(L)])
        # mean of the measurements' world coordinates (creation, and the reset of an update), added in list order
        world = _apply(C2W[None], M)
        acc = np.zeros((n, 3))
        for k in range(L):
            acc += np.where(valid[:, k, None], world[:, k], 0.0)
        n_list = valid.sum(axis=1)

        kind = np.full(n, CREATE, np.int64)
        lm = np.zeros((n, 3))
        lmup = np.zeros(n, np.int64)
        margin = np.full(n, np.inf)
        iterations = np.zeros(n, np.int64)
        create = carried_lmup == 0
        lm[create] = acc[create] / n_list[create, None]          # a list that ends early shortens the creation
        lmup[create] = n_list[create]
        upd = np.nonzero(~create)[0]
        if len(upd):
            k_, lm_, up_, mg_, it_ = self._update(M[upd], valid[upd], W2C, carried[upd], carried_lmup[upd], length[upd], acc[upd])
            kind[upd], lm[upd], lmup[upd], margin[upd], iterations[upd] = k_, lm_, up_, mg_, it_
        self.previous = (np.asarray(points["lm"], np.float64).copy(), meta[:, 4].astype(np.int64))
        return FrameResult(index, kind, n_meas, length, lm, lmup, margin, carried, carried_lmup, truncated, iterations)

    # -- Landmark::update ------------------------------------------------------------------------------------------
    def _update(self, M, valid, W2C, start, lmup0, length, acc):
        n = len(M)
        R = W2C[:, :, :3]
        RtR = np.einsum("kai,kaj->kij", R, R)
        om0 = np.where(valid, 1.0 / np.where(valid, M[:, :, 2], 1.0), 0.0)       # information: the inverse depth
        w = start.copy()
        err_prev = np.zeros(n)
        margin = np.full(n, np.inf)
        kind = np.full(n, UNFINISHED, np.int64)
        lm = start.copy()
        lmup = lmup0.copy()
        iterations = np.zeros(n, np.int64)
        active = np.ones(n, bool)
        for it in range(self.max_iterations):
            a = np.nonzero(active)[0]
            if not len(a):
                break
            s = _apply(W2C[None], w[a][:, None, :])                              # [a, L, 3] the estimate in every frame of the list
            va = valid[a]
            front = va & (s[:, :, 2] > 0)                                        # behind the camera: an outlier that adds nothing
            e = s - M[a]
            e2 = om0[a] * ((e[:, :, 0] ** 2 + e[:, :, 1] ** 2) + e[:, :, 2] ** 2)
            saturated = front & (e2 > self.kernel)
            om = np.where(saturated, om0[a] * self.kernel / np.where(saturated, e2, 1.0), om0[a]) * front
            err = np.where(front, e2, 0.0).sum(axis=1)
            n_out = (va & ~front).sum(axis=1) + saturated.sum(axis=1)
            H = np.einsum("ek,kij->eij", om, RtR)
            b = np.einsum("ek,kji,ekj->ei", om, R, e)
            solvable = np.abs(np.linalg.det(H)) > 0
            dx = np.zeros((len(a), 3))
            if solvable.any():
                dx[solvable] = np.linalg.solve(H[solvable], -b[solvable][:, :, None])[:, :, 0]
            w[a] += dx
            iterations[a] += 1
            # margins of this round's decisions
            m = np.where(solvable, np.inf, 0.0)
            m = np.minimum(m, np.where(va, np.abs(s[:, :, 2]) / np.where(va, np.abs(M[a][:, :, 2]), 1.0), np.inf).min(axis=1))
            m = np.minimum(m, np.where(front, _rel(e2, self.kernel), np.inf).min(axis=1))
            change = np.abs(err - err_prev[a])
            m = np.minimum(m, _rel(change, CONVERGENCE))
            stop = (change < CONVERGENCE) | (it == 999)
            n_in = length[a] - n_out
            accept = stop & (n_in > lmup0[a])
            reset = stop & ~accept & (n_in < n_out)
            keep = stop & ~accept & ~reset
            # integer comparisons are exact: their thresholds lie half-way between two integers
            m = np.minimum(m, np.where(stop, np.minimum(np.abs(n_in - lmup0[a] - 0.5) / np.maximum(lmup0[a], 1),
                                                        np.abs(n_in - n_out + 0.5) / np.maximum(n_out, 1)), np.inf))
            margin[a] = np.minimum(margin[a], m)
            ia = a[accept]
            lm[ia] = w[ia]; lmup[ia] = n_in[accept]; kind[ia] = ACCEPT
            ir = a[reset]
            lm[ir] = acc[ir] / length[ir, None]; kind[ir] = RESET
            kind[a[keep]] = KEEP
            err_prev[a] = err
            active[a[stop]] = False
        return kind, lm, lmup, margin, iterations


class Tally(object):
    """Compares exports with FrameResults frame by frame and counts what the run reached (the premises of a test)."""

    LENGTHS = (8, 9, 10, 16, 17, 33, 34, 35, 48, 49, 50)

    def __init__(self, update_tol=1e-9, creation_rtol=1e-12):
        self.update_tol, self.creation_rtol = update_tol, creation_rtol
        self.updates = self.creations = self.undecidable = self.truncated_updates = 0
        self.kinds = collections.Counter()
        self.truncated_kinds = collections.Counter()       # outcome of the updates whose list was cut to the ring
        self.by_n_meas = collections.Counter()             # updates by measurements of the track (track length + 1)
        self.truncated_frames = []
        self.frames = 0
        self.worst_update = self.worst_creation = 0.0

    def at_least(self, n_meas):
        return sum(v for k, v in self.by_n_meas.items() if k >= n_meas)

    def check(self, res, points, tag=""):
        """points: the export the FrameResult was computed for."""
        lm = np.asarray(points["lm"])[res.index]
        lmup = np.asarray(points["meta"])[res.index, 4]
        create = res.kind == CREATE
        update = ~create
        decided = res.margin >= MARGIN
        self.frames += 1
        self.creations += int(create.sum())
        self.updates += int(update.sum())
        self.undecidable += int((update & ~decided).sum())
        self.truncated_updates += int((update & res.truncated).sum())
        if res.truncated.any():
            self.truncated_frames.append(self.frames - 1)
        for k in res.kind[update]:
            self.kinds[KIND_NAMES[k]] += 1
        for k in res.kind[update & res.truncated]:
            self.truncated_kinds[KIND_NAMES[k]] += 1
        for k in res.n_meas[update]:
            self.by_n_meas[int(k)] += 1
        if create.any():
            self.worst_creation = max(self.worst_creation, float(np.max(np.abs(lm[create] - res.lm[create]) / np.maximum(np.abs(res.lm[create]), 1e-300))))
            np.testing.assert_allclose(lm[create], res.lm[create], rtol=self.creation_rtol, atol=0, err_msg="%s: created landmarks" % tag)
            np.testing.assert_array_equal(lmup[create], res.lmup[create], err_msg="%s: update count of created landmarks" % tag)
        j = update & decided
        if j.any():
            self.worst_update = max(self.worst_update, float(np.max(np.abs(lm[j] - res.lm[j]) / (1.0 + np.abs(res.lm[j])))))
            np.testing.assert_array_equal(lmup[j], res.lmup[j], err_msg="%s: update counts (n_meas %s, kinds %s)" % (tag, res.n_meas[j], res.kind[j]))
            np.testing.assert_allclose(lm[j], res.lm[j], rtol=self.update_tol, atol=self.update_tol, err_msg="%s: refined landmarks" % tag)
            kept = j & ((res.kind == KEEP) | (res.kind == UNFINISHED))      # out of iterations: nothing is decided, the estimate stays
            np.testing.assert_array_equal(lm[kept], res.carried[kept], err_msg="%s: a kept estimate must be the predecessor's, bit for bit" % tag)

    def summary(self):
        return dict(frames=self.frames, creations=self.creations, updates=self.updates, undecidable=self.undecidable,
                    ge9=self.at_least(9), ge34=self.at_least(34), ge49=self.at_least(49), truncated=self.truncated_updates,
                    kinds=dict(self.kinds), truncated_kinds=dict(self.truncated_kinds), max_n_meas=max(self.by_n_meas) if self.by_n_meas else 0,
                    worst_update=self.worst_update, worst_creation=self.worst_creation,
                    exact={k: self.by_n_meas.get(k, 0) for k in self.LENGTHS + (63, 64, 65)})

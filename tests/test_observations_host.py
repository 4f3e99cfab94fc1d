"""Host side of the landmark observation export (no GPU): evaluation.reprojection_residuals against a projection written out here,
exact round trips of the bundle and of the text writer, and sharding.assemble_observations against hand-built chunk maps and logs."""
import numpy as np

from vslam_pose_estimation_framework_amd import evaluation, io_formats, sharding


def _rot(axis, angle):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def _problem():
    rng = np.random.RandomState(5)
    K = np.array([[718.856, 0.0, 607.1928], [0.0, 718.856, 185.2157], [0.0, 0.0, 1.0]])
    bh = np.array([-386.1448, 0.0, 0.0])
    poses = []
    for f in range(4):
        R = _rot([0.2, 1.0, -0.1], 0.05 * f)
        t = np.array([0.3 * f, -0.02 * f, 1.1 * f])
        poses.append(np.hstack([R, t.reshape(3, 1)]))
    poses = np.array(poses)
    xyz = np.column_stack([rng.uniform(-6, 6, 12), rng.uniform(-2, 2, 12), rng.uniform(12, 40, 12)])
    obs_id = np.array([i for f in range(4) for i in range(12)], np.int32)
    obs_frame = np.array([f for f in range(4) for i in range(12)], np.int32)
    return K, bh, poses, xyz, obs_id, obs_frame


def _project(K, bh, poses, xyz, obs_id, obs_frame):
    """The projection, one observation at a time, with 4x4 matrices: independent of reprojection_residuals' arithmetic."""
    out = np.zeros((len(obs_id), 4))
    for n, (i, f) in enumerate(zip(obs_id, obs_frame)):
        T = np.eye(4)
        T[:3, :] = poses[f]
        p = (np.linalg.inv(T) @ np.append(xyz[i], 1.0))[:3]
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        out[n, 0] = fx * p[0] / p[2] + cx
        out[n, 1] = fy * p[1] / p[2] + cy
        out[n, 2] = (fx * p[0] + cx * p[2] + bh[0]) / (p[2] + bh[2])
        out[n, 3] = out[n, 1]
    return out


def test_reprojection_residuals_known_answer():
    K, bh, poses, xyz, obs_id, obs_frame = _problem()
    kp = _project(K, bh, poses, xyz, obs_id, obs_frame)
    res, valid = evaluation.reprojection_residuals(K, bh, poses.reshape(-1, 12), xyz, obs_id, obs_frame, kp)
    assert res.shape == (48, 3) and valid.shape == (48,) and valid.all()
    assert np.abs(res).max() < 1e-9
    # one perturbed pixel comes back as its own residual (du_L, dv, du_R), the others stay at zero
    kp2 = kp.copy()
    kp2[17] += [2.0, -1.0, 3.0, -1.0]
    res2, valid2 = evaluation.reprojection_residuals(K, bh, poses, xyz, obs_id, obs_frame, kp2)
    assert valid2.all()
    assert np.abs(res2[17] - [2.0, -1.0, 3.0]).max() < 1e-9
    assert np.abs(np.delete(res2, 17, axis=0)).max() < 1e-9
    # the right camera sits baseline metres to the right: the same point has the smaller column there
    assert (kp[:, 2] < kp[:, 0]).all()


def test_reprojection_residuals_masks_points_behind_the_camera():
    K, bh, poses, xyz, obs_id, obs_frame = _problem()
    xyz = xyz.copy()
    xyz[3] = poses[2][:, :3] @ np.array([0.5, 0.1, -4.0]) + poses[2][:, 3]      # 4 m behind frame 2's camera
    kp = np.zeros((len(obs_id), 4))
    res, valid = evaluation.reprojection_residuals(K, bh, poses, xyz, obs_id, obs_frame, kp)
    n = 2 * 12 + 3
    assert not valid[n] and np.isnan(res[n]).all()
    keep = np.ones(len(obs_id), bool)
    keep[obs_id == 3] = False
    assert valid[keep].all() and np.isfinite(res[keep]).all()


def _map_of(first, last, seed):
    rng = np.random.RandomState(seed)
    n = len(first)
    return dict(id=np.arange(n, dtype=np.int32), xyz=rng.uniform(-5, 5, (n, 3)), first_frame=np.array(first, np.int32),
                last_frame=np.array(last, np.int32), updates=rng.randint(1, 9, n).astype(np.int32), desc=rng.randint(0, 256, (n, 32)).astype(np.uint8))


def _log_of(m, seed):
    """Every landmark seen in every frame first_frame .. last_frame, sorted by frame and then by id (a stand-in for point order)."""
    rng = np.random.RandomState(seed)
    rows = sorted((f, i) for i in range(len(m["id"])) for f in range(m["first_frame"][i], m["last_frame"][i] + 1))
    return dict(id=np.array([i for f, i in rows], np.int32), frame=np.array([f for f, i in rows], np.int32),
                kp=rng.randint(0, 1200, (len(rows), 4)).astype(np.int16))


def test_bundle_round_trip_is_exact(tmp_path):
    rng = np.random.RandomState(2)
    m = _map_of([0, 0, 2, 3], [4, 1, 5, 3], 1)
    obs = _log_of(m, 2)
    K = np.array([[700.5, 0, 600.25], [0, 701.5, 180.75], [0, 0, 1]])
    bh = np.array([-380.123456789, 0.0, 0.0])
    poses = rng.standard_normal((6, 12))
    path = str(tmp_path / "bundle.npz")
    io_formats.write_bundle(path, K, bh, poses, m, obs)
    b = io_formats.read_bundle(path)
    for got, want in ((b["K"], K), (b["baseline_h"], bh), (b["poses"], poses), (b["obs_id"], obs["id"]), (b["obs_frame"], obs["frame"]),
                      (b["obs_kp"], obs["kp"])):
        assert got.dtype == np.asarray(want).dtype
        np.testing.assert_array_equal(got, want)
    assert b["poses"].shape == (6, 12) and b["obs_kp"].shape == (len(obs["id"]), 4) and b["obs_kp"].dtype == np.int16
    assert sorted(b["map"]) == sorted(m)
    for k in m:
        assert b["map"][k].dtype == m[k].dtype
        np.testing.assert_array_equal(b["map"][k], m[k])
    # an assembled map carries `chunk` and may come without descriptors
    m2 = {k: v for k, v in m.items() if k != "desc"}
    m2["chunk"] = np.array([0, 0, 1, 1], np.int32)
    io_formats.write_bundle(path, K, bh, poses.reshape(6, 3, 4), m2, obs)
    b2 = io_formats.read_bundle(path)
    assert sorted(b2["map"]) == sorted(m2)
    np.testing.assert_array_equal(b2["map"]["chunk"], m2["chunk"])
    np.testing.assert_array_equal(b2["poses"], poses)


def test_observations_text_round_trip(tmp_path):
    m = _map_of([0, 1, 1], [3, 2, 4], 3)
    obs = _log_of(m, 4)
    obs["kp"][0] = [-3, 0, 32767, -32768]
    path = str(tmp_path / "obs.txt")
    io_formats.write_observations_text(path, obs["id"], obs["frame"], obs["kp"])
    lines = open(path).read().splitlines()
    assert len(lines) == len(obs["id"])
    rows = np.array([[int(v) for v in ln.split()] for ln in lines])
    assert rows.shape == (len(obs["id"]), 6)
    np.testing.assert_array_equal(rows[:, 0], obs["frame"])
    np.testing.assert_array_equal(rows[:, 1], obs["id"])
    np.testing.assert_array_equal(rows[:, 2:], obs["kp"])
    assert list(rows[:, 0]) == sorted(rows[:, 0])              # the log's order: by frame


def test_assemble_observations_synthetic_plan():
    plan, L = sharding.plan_chunks(30, 3, 3)
    assert plan == [(0, 0, 10), (7, 10, 20), (17, 20, 30)]
    # chunk-local frames.  Chunk 1 (start 7): landmarks 0 and 1 are created in the warm-up (global 7 and 9) -> duplicates;
    # 2, 3, 4 are created at global 10, 12, 19 -> kept.  Chunk 2 (start 17): landmark 0 warm-up (global 19), 1 and 2 kept (20, 29).
    maps = [_map_of([0, 0, 4, 9], [9, 2, 6, 9], 10),
            _map_of([0, 2, 3, 5, 12], [8, 12, 7, 5, 12], 11),
            _map_of([2, 3, 12], [11, 4, 12], 12)]
    logs = [_log_of(m, 20 + c) for c, m in enumerate(maps)]
    poses = []
    for c, (st, fi, en) in enumerate(plan):
        P = np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]), (en - st, 1, 1))
        P[:, 2, 3] = np.arange(en - st) + 0.25 * c
        poses.append(P)
    before = sharding.assemble_map(maps, poses, plan)
    out = sharding.assemble_observations(maps, logs, plan)
    after = sharding.assemble_map(maps, poses, plan)
    for k in before:
        np.testing.assert_array_equal(before[k], after[k])
    assert list(before["chunk"]) == [0, 0, 0, 0, 1, 1, 1, 2, 2]
    # expected: per chunk, the rows of kept landmarks, renumbered in chunk order, frames + start
    kept = [[0, 1, 2, 3], [2, 3, 4], [1, 2]]
    base, want_id, want_frame, want_kp, want_chunk, dropped = 0, [], [], [], [], 0
    for c, (st, fi, en) in enumerate(plan):
        new = {old: base + j for j, old in enumerate(kept[c])}
        base += len(kept[c])
        for i, f, k in zip(logs[c]["id"], logs[c]["frame"], logs[c]["kp"]):
            if int(i) in new:
                want_id.append(new[int(i)]); want_frame.append(int(f) + st); want_kp.append(k); want_chunk.append(c)
            else:
                dropped += 1
    np.testing.assert_array_equal(out["id"], want_id)
    np.testing.assert_array_equal(out["frame"], want_frame)
    np.testing.assert_array_equal(out["kp"], np.array(want_kp))
    np.testing.assert_array_equal(out["chunk"], want_chunk)
    assert out["dropped"] == dropped == (9 + 11) + 10
    assert out["id"].dtype == np.int32 and out["frame"].dtype == np.int32 and out["kp"].dtype == np.int16
    # ids line up with assemble_map's: every id exists, and its frames are exactly first_frame .. last_frame of that entry
    assert set(out["id"]) == set(before["id"])
    for i in before["id"]:
        fr = out["frame"][out["id"] == i]
        assert list(fr) == list(range(before["first_frame"][i], before["last_frame"][i] + 1))
        assert (out["chunk"][out["id"] == i] == before["chunk"][i]).all()
    # frames of a kept observation lie in its chunk's own range, so the assembled log is sorted by frame
    assert list(out["frame"]) == sorted(out["frame"])
    # a chunk behind the end of the sequence is skipped, as in assemble_map
    plan4, _ = sharding.plan_chunks(30, 4, 3)
    plan4[3] = (30, 30, 30)
    out4 = sharding.assemble_observations(maps + [_map_of([], [], 0)], logs + [dict(id=[], frame=[], kp=np.zeros((0, 4), np.int16))],
                                          plan[:3] + [plan4[3]])
    np.testing.assert_array_equal(out4["id"], out["id"])
    np.testing.assert_array_equal(out4["frame"], out["frame"])

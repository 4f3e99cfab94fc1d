"""Host side of the landmark map: the C ABI exports it, the PLY writer / reader round-trips exactly, and sharding.assemble_map
brings chunk maps into one world through the seam transforms of assemble_trajectory (which stays as it was)."""
import ctypes
import os

import numpy as np

from vslam_pose_estimation_framework_amd import hip, io_formats, sharding
from vslam_pose_estimation_framework_amd.evaluation import inv34, mul34


def test_library_exports_map_entry_points():
    lib = ctypes.CDLL(hip.lib_path())
    for name in ("vslam_enable_map", "vslam_get_map_size", "vslam_get_map"):
        assert hasattr(lib, name), name


def test_ply_round_trip_is_exact(tmp_path):
    rng = np.random.default_rng(3)
    n = 1000
    xyz = rng.normal(size=(n, 3)) * 10 ** rng.uniform(-8, 4, size=(n, 1))
    xyz[0] = [np.pi, -0.0, 1e-300]
    ints = dict(id=np.arange(n), first_frame=rng.integers(0, 5000, n), last_frame=rng.integers(0, 5000, n),
                updates=rng.integers(-2 ** 31, 2 ** 31 - 1, n))
    p = str(tmp_path / "m.ply")
    io_formats.write_ply(p, xyz, **ints)
    with open(p, "rb") as f:
        head = f.read(200)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\n")
    back = io_formats.read_ply(p)
    assert back["xyz"].dtype == np.float64
    np.testing.assert_array_equal(back["xyz"].view(np.uint64), xyz.view(np.uint64))     # bit for bit, -0.0 included
    for k, v in ints.items():
        np.testing.assert_array_equal(back[k], v)
    assert os.path.getsize(p) == len(open(p, "rb").read().split(b"end_header\n", 1)[0]) + len(b"end_header\n") + n * (3 * 8 + 4 * 4)
    empty = str(tmp_path / "e.ply")
    io_formats.write_ply(empty, np.zeros((0, 3)))
    e = io_formats.read_ply(empty)
    assert e["xyz"].shape == (0, 3) and e["id"].shape == (0,)


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def _trajectory(n, rng):
    T = np.zeros((n, 3, 4))
    for f in range(n):
        T[f, :, :3] = _rot(0.01 * f, 0.03 * f + 0.1 * np.sin(0.2 * f), 0.005 * f)
        T[f, :, 3] = [np.sin(0.1 * f), 0.05 * f, 0.9 * f]
    return T


def test_assemble_map_recovers_the_cloud():
    rng = np.random.default_rng(5)
    total, n_chunks, overlap = 47, 4, 5
    G = _trajectory(total, rng)
    plan, _ = sharding.plan_chunks(total, n_chunks, overlap)
    # a global map: landmark j created at frame first[j] and last updated at last[j]
    m = 600
    first = rng.integers(0, total, m)
    last = np.minimum(first + rng.integers(0, 12, m), total - 1)
    cloud = rng.uniform(-20, 20, (m, 3))
    chunk_maps, chunk_poses, expect = [], [], []
    for c, (start, fu, end) in enumerate(plan):
        # the chunk's world: its own first frame is the origin (what a fresh stream estimates), poses exact up to that change of frame
        W = inv34(G[start])                                  # global -> chunk world
        chunk_poses.append(np.array([mul34(W, G[f]) for f in range(start, end)]))
        # the chunk sees every landmark created in start .. end-1: warm-up ones are duplicates of the preceding chunk's
        sel = np.nonzero((first >= start) & (first < end))[0]
        sel = sel[rng.permutation(len(sel))]                  # chunk-local ids in some order of their own
        xyz = cloud[sel] @ W[:, :3].T + W[:, 3]
        chunk_maps.append(dict(id=np.arange(len(sel)), xyz=xyz, first_frame=first[sel] - start, last_frame=np.minimum(last[sel], end - 1) - start,
                               updates=sel.astype(np.int32) + 1, desc=np.repeat(sel.astype(np.uint8)[:, None], 32, 1)))
        expect.append(sel[(first[sel] >= fu) & (first[sel] < end)])
    out = sharding.assemble_map(chunk_maps, chunk_poses, plan, seam_frames=1)
    want = np.concatenate(expect)
    assert len(out["id"]) == len(want) == m                  # every landmark once: no warm-up duplicates
    assert sorted(out["updates"] - 1) == list(range(m))
    np.testing.assert_allclose(out["xyz"], cloud[want], rtol=0, atol=1e-9)
    np.testing.assert_array_equal(out["first_frame"], first[want])
    assert np.all(out["last_frame"] >= out["first_frame"]) and out["last_frame"].max() < total
    np.testing.assert_array_equal(out["id"], np.arange(m))
    np.testing.assert_array_equal(out["desc"][:, 0], want.astype(np.uint8))
    for c, (start, fu, end) in enumerate(plan):
        ff = out["first_frame"][out["chunk"] == c]
        assert np.all((ff >= fu) & (ff < end))
    # more seam frames: the same cloud (the chunk poses are exact)
    out3 = sharding.assemble_map(chunk_maps, chunk_poses, plan, seam_frames=3)
    np.testing.assert_allclose(out3["xyz"], cloud[want], rtol=0, atol=1e-9)


def _assemble_trajectory_as_before(chunk_poses, plan, seam_frames=1):
    total = plan[-1][2]
    G = np.zeros((total, 3, 4))
    anchor = np.hstack([np.eye(3), np.zeros((3, 1))])
    for c, (start, first, end) in enumerate(plan):
        P = np.asarray(chunk_poses[c]).reshape(-1, 3, 4)
        if end <= first:
            continue
        if c > 0 and first > start:
            anchor = sharding._seam_anchor(G, P, start, first, seam_frames)
        elif c > 0:
            anchor = mul34(G[first - 1], inv34(P[0])) if first > 0 else anchor
        for f in range(first, end):
            G[f] = mul34(anchor, P[f - start])
    return G


def test_assemble_trajectory_unchanged():
    rng = np.random.default_rng(9)
    for total, n_chunks, overlap, seam in ((47, 4, 5, 1), (100, 7, 6, 3), (30, 3, 0, 1), (12, 5, 2, 2), (4541, 160, 6, 1)):
        plan, _ = sharding.plan_chunks(total, n_chunks, overlap)
        chunks = []
        for (start, fu, end) in plan:
            k = max(end - start, 0)
            P = np.zeros((k, 3, 4))
            for f in range(k):
                P[f, :, :3] = _rot(*(rng.normal(size=3) * 0.1))
                P[f, :, 3] = rng.normal(size=3) * 5
            chunks.append(P)
        got = sharding.assemble_trajectory(chunks, plan, seam_frames=seam)
        want = _assemble_trajectory_as_before(chunks, plan, seam_frames=seam)
        np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))

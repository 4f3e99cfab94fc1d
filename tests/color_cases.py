"""What the colour-input tests share (test_gray_host.py, test_gray_gpu.py, test_rgbd_gray_gpu.py, test_run_color.py): colour frames made
from the renderer's grey ones, their views in the four pixel formats, the rounding-tie triples, and folders of colour PNGs."""
import numpy as np

from vslam_pose_estimation_framework_amd import color

# (R, G, B) whose weighted sum lies exactly on, or just below, a half: (0, 56, 102) -> 44.5 -> 45, (0, 116, 65) -> 75.5 -> 76,
# (0, 47, 8) -> 28.49994 -> 28, (0, 99, 249) -> 86.49994 -> 86
TIE_TRIPLES = np.array([(0, 56, 102), (0, 116, 65), (0, 47, 8), (0, 99, 249)], np.uint8)
TIE_GRAYS = np.array([45, 76, 28, 86], np.uint8)

STEREO_SEEDS = (7, 9, 11)
STEREO_FRAMES = 8
RGBD_SEEDS = (26, 33, 40)        # the worlds of the RGB-D cases (test_rgbd_equalize_gpu.py's scenes at full contrast)
RGBD_FRAMES = 12


def colourise(g, rng):
    """A grey image as a camera with a warm cast would have seen it: R = 1.15 g, G = g, B = 0.70 g, plus an independent integer noise in
    -6 .. 6 per channel; rint, clipped to 0 .. 255.  uint8 [..., 3] in RGB order."""
    g = np.asarray(g).astype(np.float64)
    rgb = np.stack([1.15 * g, g, 0.70 * g], axis=-1) + rng.integers(-6, 7, g.shape + (3,))
    return np.clip(np.rint(rgb), 0, 255).astype(np.uint8)


def as_format(rgb, fmt, rng=None):
    """The RGB array in pixel format fmt: channels reversed for the BGR formats, an alpha plane of random bytes appended for the
    four-channel ones."""
    rgb = np.asarray(rgb)
    out = rgb if fmt in (color.RGB8, color.RGBA8) else rgb[..., ::-1]
    if color.channels(fmt) == 4:
        rng = rng or np.random.default_rng(5)
        out = np.concatenate([out, rng.integers(0, 256, rgb.shape[:-1] + (1,)).astype(np.uint8)], axis=-1)
    return np.ascontiguousarray(out)


def stereo_colour_frames(o, scenes, frames=STEREO_FRAMES):
    """Per frame (L, R): RGB arrays [n_scenes, rows, cols, 3]; scene s is colourised with default_rng(100 + its seed), drawn left then
    right each frame."""
    rngs = [np.random.default_rng(100 + int(sc.seed)) for sc in scenes]
    out = []
    for k in range(frames):
        Ls, Rs = [], []
        for sc, rng in zip(scenes, rngs):
            L, R = o.render(sc, k)
            Ls.append(colourise(L, rng)); Rs.append(colourise(R, rng))
        out.append((np.stack(Ls), np.stack(Rs)))
    return out


def rgbd_world(o, seed, frames=RGBD_FRAMES):
    """The tum configuration at 620 x 188 on the street scene of `seed`: (cfg, p, K, [(RGB image, depth, its grey)])."""
    import undistort_cases as uc
    from test_rgbd_mode import setup
    scene, cfg, p = setup(o, "tum", descriptor=1, seed=seed)
    rng = np.random.default_rng(200 + seed)
    out = []
    for L, D in uc.render_frames(o, scene, frames):
        c = colourise(L, rng)
        out.append((c, D, color.to_gray_u8(c, color.RGB8)))
    K = np.array([[scene.fx, 0, scene.cx], [0, scene.fy, scene.cy], [0, 0, 1.0]])
    return cfg, p, K, out


def reregistration_scenario(o):
    """The scenario of test_rgbd_reregistration_paths (icl configuration, a jump from frame 8 to frame 16) on colourised frames: (cfg, p,
    [(RGB image, depth)]).  The landmark minimum is 15 here (30 in the grey scenario): under the colourised frames' noise the icl
    configuration holds 20 - 50 landmarks, and with 30 it never leaves LOCALIZING, where nothing is registered twice.  Chosen on the
    checker loop alone: attempts 0 1 1 1 2 2 1 2 1 3 1 1 (test_gray_host.py asserts it)."""
    import undistort_cases as uc
    from test_rgbd_mode import setup
    scene, cfg, p = setup(o, "icl", descriptor=0, max_depth=30.0, seed=41)
    cfg.minimum_number_of_landmarks_to_track = 15
    rng = np.random.default_rng(241)
    return cfg, p, [(colourise(o.render(scene, k)[0], rng), o.render_depth(scene, k, uc.DEPTH_UNIT)) for k in [0, 1, 2, 3, 4, 5, 6, 7, 8, 16, 17, 18]]


def write_tum_folder_color(root, frames, skew=0.004):
    """A TUM RGB-D folder whose rgb/ images are the given RGB arrays: frames = [(RGB [rows, cols, 3], depth u16)]."""
    from vslam_pose_estimation_framework_amd import io_formats as io
    (root / "rgb").mkdir(parents=True); (root / "depth").mkdir()
    rgb_lines, dep_lines = ["# color images", "# timestamp filename"], ["# depth maps"]
    for k, (c, D) in enumerate(frames):
        t = 1305031100.0 + k / 30.0
        io.write_png(str(root / "rgb" / ("%.6f.png" % t)), c)
        io.write_png(str(root / "depth" / ("%.6f.png" % (t + skew))), D)
        rgb_lines.append("%.6f rgb/%.6f.png" % (t, t)); dep_lines.append("%.6f depth/%.6f.png" % (t + skew, t + skew))
    (root / "rgb.txt").write_text("\n".join(rgb_lines) + "\n")
    (root / "depth.txt").write_text("\n".join(dep_lines) + "\n")


def kitti_calib_text(scene, wrong=2.0):
    """calib.txt with P0 .. P3: the colour pair (2, 3) carries the scene's rig, its left camera 0.06 m off the rig's origin as on the
    car; the grey pair (0, 1) carries a baseline `wrong` times as long, so that reading the wrong lines cannot go unnoticed."""
    fx, fy, cx, cy, b = (float(v) for v in (scene.fx, scene.fy, scene.cx, scene.cy, scene.baseline_m))
    rows = [("P0", 0.0), ("P1", -fx * b * wrong), ("P2", fx * 0.06), ("P3", fx * 0.06 - fx * b)]
    return "".join("%s: %r 0 %r %r 0 %r %r 0 0 0 1 0\n" % (n, fx, cx, tx, fy, cy) for n, tx in rows)

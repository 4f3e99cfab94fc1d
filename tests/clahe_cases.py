"""Shared inputs of the CLAHE tests: the unevenly lit scene (a column ramp over the low-contrast KITTI-like scene), numpy CLAHE on pairs
and batches, and the (rows, cols, tilesX, tilesY, clip) list both the host and the device comparison run on."""
import numpy as np

from vslam_pose_estimation_framework_amd import clahe

CLIP, TILES = 40.0, (8, 8)
FRAMES = 8
SEEDS = (7, 9, 11)

# (rows, cols, tilesX, tilesY, clipLimit): both-dimensions-indivisible, whole tiles, the clip-1 floor (0.001), and the two shapes where
# only one dimension is indivisible and the other one still grows by a full tile count
SHAPES = [(9, 9, 8, 8, 40), (2, 3, 1, 1, 0), (16, 24, 8, 8, 2), (24, 17, 8, 8, 4), (17, 24, 8, 8, 40), (61, 67, 4, 2, 3), (61, 67, 3, 5, 0.001),
          (12, 10, 5, 3, 40), (4, 8, 4, 2, 0), (6, 8, 4, 2, 1000)]


def contents(rng, rows, cols):
    """(name, image) of the three contents every shape runs with."""
    return [("random", rng.integers(0, 256, (rows, cols)).astype(np.uint8)),
            ("constant", np.full((rows, cols), int(rng.integers(0, 256)), np.uint8)),
            ("100..120", rng.integers(100, 121, (rows, cols)).astype(np.uint8))]


def shade(img):
    """Every row multiplied by a column ramp from 0.15 to 1.0 (float64, rint, clipped to u8): the left of the frame is dim."""
    ramp = np.linspace(0.15, 1.0, img.shape[-1])
    return np.clip(np.rint(img.astype(np.float64) * ramp), 0, 255).astype(np.uint8)


def shaded_scene(o, seed=7):
    scene = o.scene_kitti(scale=0.4, seed=seed)
    scene.contrast = 0.3
    return scene


def render_shaded(o, scenes, k):
    """uint8 [B, rows, cols] left and right of frame k of every scene, shaded."""
    imgs = [o.render(sc, k) for sc in scenes]
    return np.ascontiguousarray(np.stack([shade(p[0]) for p in imgs])), np.ascontiguousarray(np.stack([shade(p[1]) for p in imgs]))


def clahe_image(img, clip=CLIP, tiles=TILES):
    return clahe.clahe_u8(img, clip, tiles)[0]


def clahe_batch(L, clip=CLIP, tiles=TILES):
    return np.ascontiguousarray(np.stack([clahe_image(x, clip, tiles) for x in L]))


def rgbd_shaded_frames(o, seed, n=12):
    """The tum configuration of test_rgbd_mode.setup at 188 x 620 (neither divisible by 8) and contrast 0.3, shaded:
    -> (cfg, params, K, [(image, depth)])."""
    import undistort_cases as uc
    from test_rgbd_mode import setup
    scene, cfg, p = setup(o, "tum", descriptor=1, seed=seed)
    scene.contrast = 0.3
    K = np.array([[scene.fx, 0, scene.cx], [0, scene.fy, scene.cy], [0, 0, 1.0]])
    return cfg, p, K, [(shade(L), D) for L, D in uc.render_frames(o, scene, n)]

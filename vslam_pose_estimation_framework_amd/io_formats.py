"""Data formats on either side of the hot path.

* KITTI odometry folder (`image_0/`, `image_1/`, `calib.txt`, `times.txt`) -> stereo pairs + camera values, with the
  calibration parsed exactly like the reference's harness (executables/test_stereo_frontend.cpp:281-312: first line =
  left projection matrix P0 -> fx, cx, fy, cy; second line P1 -> b_x = P1(0,3)).
* trajectory writers equal to WorldMap::writeTrajectoryKITTI / writeTrajectoryTUM (src/types/world_map.cpp:184-258):
  fixed notation, 9 digits, one trailing blank before the newline.
* a dependency-free reader/writer for 8-bit grayscale PNG (what KITTI ships): no OpenCV/PIL in this image; the general reader
  (8 / 16-bit grayscale, 8-bit RGB / RGBA) serves the RGB-D data sets.
* TUM RGB-D folder (`rgb.txt`, `depth.txt`, `rgb/`, `depth/`, optional `groundtruth.txt`; also how ICL-NUIM is distributed) -> gray image +
  16-bit depth pairs, associated on time stamps like the benchmark's associate.py."""
import os
import struct
import zlib

import numpy as np


# ---- KITTI calibration -------------------------------------------------------------------------------------
def parse_kitti_calib(path, cameras=(0, 1)):
    """Returns (K 3x3, baseline_homogeneous 3) as getCameraCalibrationMatrixKITTI does (the grey pair, cameras 0 and 1: the file's first
    two lines).  Another pair, e.g. the colour cameras (2, 3): the lines are found by their `P2:` / `P3:` labels, K comes from the left
    camera's matrix and baseline[0] is the difference of the two matrices' [0, 3] entries (the left one need not be the rig's origin)."""
    with open(path) as f:
        lines = [ln for ln in f.read().splitlines()]
    if not lines or not lines[0].strip():
        raise RuntimeError("invalid camera calibration file provided")
    if tuple(cameras) != (0, 1):
        rows = {}
        for ln in lines:
            a = ln.split()
            if a and a[0].endswith(":") and len(a) >= 13:
                rows[a[0][:-1]] = [float(v) for v in a[1:13]]
        try:
            pl, pr = rows["P%d" % cameras[0]], rows["P%d" % cameras[1]]
        except KeyError as e:
            raise RuntimeError("camera calibration file has no line %s: %s" % (e, path))
        K = np.eye(3)
        K[0, 0] = pl[0]; K[0, 2] = pl[2]; K[1, 1] = pl[5]; K[1, 2] = pl[6]
        baseline = np.zeros(3)
        baseline[0] = pr[3] - pl[3]
        return K, baseline
    a = lines[0].split()      # "P0:" fx 0 cx 0 0 fy cy 0 0 0 1 0
    K = np.eye(3)
    K[0, 0] = float(a[1]); K[0, 2] = float(a[3]); K[1, 1] = float(a[6]); K[1, 2] = float(a[7])
    b = lines[1].split()      # "P1:" fx 0 cx bx ...
    baseline = np.zeros(3)
    baseline[0] = float(b[4])
    return K, baseline


def apply_calib(cfg, K, baseline, rows, cols):
    cfg.rows, cfg.cols = int(rows), int(cols)
    for i in range(9):
        cfg.K[i] = float(K.reshape(9)[i])
    for i in range(3):
        cfg.baseline_h[i] = float(baseline[i])
    return cfg


# ---- minimal PNG (8-bit grayscale, non-interlaced) --------------------------------------------------------------
def write_png_gray8(path, img):
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(h))

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def read_png_gray8(path):
    data = open(path, "rb").read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise RuntimeError("not a PNG: " + path)
    pos, idat, w = 8, [], None
    while pos < len(data):
        n, t = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        pos += 12 + n
        if t == b"IHDR":
            w, h, depth, ctype, _, _, interlace = struct.unpack(">IIBBBBB", body)
            if depth != 8 or ctype != 0 or interlace != 0:
                raise RuntimeError("only 8-bit grayscale non-interlaced PNG is supported: " + path)
        elif t == b"IDAT":
            idat.append(body)
        elif t == b"IEND":
            break
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8).reshape(h, w + 1)
    out = np.zeros((h, w), np.uint8)
    prev = np.zeros(w, np.int32)
    for y in range(h):
        ft = int(raw[y, 0])
        line = raw[y, 1:].astype(np.int32)
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 255
        elif ft == 1:
            cur = np.cumsum(line) & 255
        else:  # 3 (average) and 4 (Paeth) are sequential in x
            cur = np.zeros(w, np.int32)
            left = 0
            upleft = 0
            for x in range(w):
                up = int(prev[x])
                if ft == 3:
                    pred = (left + up) >> 1
                else:
                    p = left + up - upleft
                    pa, pb, pc = abs(p - left), abs(p - up), abs(p - upleft)
                    pred = left if (pa <= pb and pa <= pc) else (up if pb <= pc else upleft)
                left = (int(line[x]) + pred) & 255
                cur[x] = left
                upleft = up
        out[y] = cur
        prev = cur
    return out


# ---- general PNG reader / writer (non-interlaced; gray 8 / 16 bit, RGB / RGBA 8 bit) ----------------------------------------------------
def _png_chunk(t, d):
    return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)


def write_png(path, img):
    """img: (h, w) uint8 | (h, w) uint16 (big-endian samples in the file, as PNG wants) | (h, w, 3) uint8."""
    img = np.asarray(img)
    if img.ndim == 2 and img.dtype == np.uint16:
        h, w = img.shape; depth, ctype = 16, 0
        rows = img.astype(">u2")
    elif img.ndim == 2:
        h, w = img.shape; depth, ctype = 8, 0
        rows = np.ascontiguousarray(img, np.uint8)
    elif img.ndim == 3 and img.shape[2] == 3:
        h, w = img.shape[:2]; depth, ctype = 8, 2
        rows = np.ascontiguousarray(img, np.uint8)
    else:
        raise ValueError("write_png: unsupported array")
    raw = b"".join(b"\x00" + rows[y].tobytes() for y in range(h))
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 0)) +
                _png_chunk(b"IDAT", zlib.compress(raw, 6)) + _png_chunk(b"IEND", b""))


def _png_unfilter(raw, h, stride, bpp):
    """Reverses the five PNG row filters; raw: h rows of 1 + stride bytes; bpp: bytes per complete pixel."""
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.int32)
    for y in range(h):
        ft = int(raw[y, 0])
        line = raw[y, 1:].astype(np.int32)
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 255
        elif ft == 1:        # Sub: a running sum per byte lane of the pixel
            cur = line.copy()
            for o in range(bpp):
                cur[o::bpp] = np.cumsum(line[o::bpp]) & 255
        else:                # 3 (average) and 4 (Paeth) are sequential in x
            cur = np.zeros(stride, np.int32)
            for x in range(stride):
                left = int(cur[x - bpp]) if x >= bpp else 0
                up = int(prev[x])
                upleft = int(prev[x - bpp]) if x >= bpp else 0
                if ft == 3:
                    pred = (left + up) >> 1
                elif ft == 4:
                    pp = left + up - upleft
                    pa, pb, pc = abs(pp - left), abs(pp - up), abs(pp - upleft)
                    pred = left if (pa <= pb and pa <= pc) else (up if pb <= pc else upleft)
                else:
                    raise RuntimeError("bad PNG filter type %d" % ft)
                cur[x] = (int(line[x]) + pred) & 255
        out[y] = cur
        prev = cur
    return out


def read_png(path):
    """(h, w) uint8 / uint16 for grayscale, (h, w, 3 | 4) uint8 for RGB / RGBA; non-interlaced files only."""
    data = open(path, "rb").read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise RuntimeError("not a PNG: " + path)
    pos, idat, hdr = 8, [], None
    while pos < len(data):
        n, t = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        pos += 12 + n
        if t == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif t == b"IDAT":
            idat.append(body)
        elif t == b"IEND":
            break
    if hdr is None:
        raise RuntimeError("PNG without IHDR: " + path)
    w, h, depth, ctype, _, _, interlace = hdr
    channels = {0: 1, 2: 3, 6: 4}.get(ctype)
    if interlace != 0 or channels is None or depth not in (8, 16) or (depth == 16 and channels != 1):
        raise RuntimeError("unsupported PNG (colour type %d, %d bit, interlace %d): %s" % (ctype, depth, interlace, path))
    bpp = channels * depth // 8
    stride = w * bpp
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8).reshape(h, stride + 1)
    px = _png_unfilter(raw, h, stride, bpp)
    if depth == 16:
        return px.reshape(h, w, 2).astype(np.uint16)[:, :, 0] * 256 + px.reshape(h, w, 2)[:, :, 1]
    return px.reshape(h, w) if channels == 1 else px.reshape(h, w, channels)


def rgb_to_gray_opencv(rgb):
    """cv::imread(..., IMREAD_GRAYSCALE) / cvtColor(BGR2GRAY) on 8-bit data [recalled: fixed point, 14 fractional bits]:
    (R * 4899 + G * 9617 + B * 1868 + 8192) >> 14."""
    a = np.asarray(rgb).astype(np.int32)
    return ((a[:, :, 0] * 4899 + a[:, :, 1] * 9617 + a[:, :, 2] * 1868 + 8192) >> 14).astype(np.uint8)


# ---- TUM RGB-D folder ----------------------------------------------------------------------------------------------------------------
# The RGB-D benchmark's camera intrinsics (fx, fy, cx, cy) and its 16-bit depth unit (1 / 5000 m); ICL-NUIM is distributed in the same layout.
TUM_INTRINSICS = {"freiburg1": (517.3, 516.5, 318.6, 255.3), "freiburg2": (520.9, 521.0, 325.1, 249.7), "freiburg3": (535.4, 539.2, 320.1, 247.6),
                  "icl": (481.2, 480.0, 319.5, 239.5)}
# the lens distortion (k1, k2, p1, p2, k3) that belongs to these camera matrices, as the benchmark's calibration page lists it [recalled];
# freiburg3's images and ICL-NUIM's renderings come undistorted.  rectify.undistortion() / tools/run_rgbd.py --undistort apply it.
TUM_DISTORTION = {"freiburg1": (0.2624, -0.9531, -0.0054, 0.0026, 1.1633), "freiburg2": (0.2312, -0.7849, -0.0033, -0.0001, 0.9172),
                  "freiburg3": (0.0, 0.0, 0.0, 0.0, 0.0), "icl": (0.0, 0.0, 0.0, 0.0, 0.0)}
TUM_DEPTH_UNIT_M = 1.0 / 5000.0


def read_tum_list(path):
    """`timestamp value...` lines, `#` comments: [(float timestamp, [tokens])]."""
    out = []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line or line[0] == "#":
                continue
            a = line.replace(",", " ").split()
            out.append((float(a[0]), a[1:]))
    return out


def associate(first, second, max_difference=0.02, offset=0.0):
    """The benchmark's associate.py: all pairs closer than max_difference, best first, every time stamp used once; sorted by the first."""
    cand = sorted((abs(a - (b + offset)), i, j) for i, a in enumerate(first) for j, b in enumerate(second) if abs(a - (b + offset)) < max_difference)
    used_a, used_b, pairs = set(), set(), []
    for _, i, j in cand:
        if i not in used_a and j not in used_b:
            used_a.add(i); used_b.add(j); pairs.append((i, j))
    return sorted(pairs)


class TumRgbdSequence(object):
    """`<root>/rgb.txt`, `<root>/depth.txt` (`timestamp path`), images under `<root>/rgb/`, `<root>/depth/`; optional
    `<root>/groundtruth.txt` (`timestamp tx ty tz qx qy qz qw`: the trajectory_analyzer's TUM format).  frame(k) = (gray u8, depth u16)."""

    def __init__(self, root, max_difference=0.02):
        self.root = root
        rgb = read_tum_list(os.path.join(root, "rgb.txt"))
        dep = read_tum_list(os.path.join(root, "depth.txt"))
        pairs = associate([t for t, _ in rgb], [t for t, _ in dep], max_difference)
        self.times = [rgb[i][0] for i, _ in pairs]
        self.rgb = [rgb[i][1][0] for i, _ in pairs]
        self.depth = [dep[j][1][0] for _, j in pairs]
        gt = os.path.join(root, "groundtruth.txt")
        self.ground_truth_path = gt if os.path.exists(gt) else None

    def __len__(self):
        return len(self.times)

    def frame(self, k):
        img = read_png(os.path.join(self.root, self.rgb[k]))
        gray = rgb_to_gray_opencv(img[:, :, :3]) if img.ndim == 3 else (img if img.dtype == np.uint8 else (img >> 8).astype(np.uint8))
        depth = read_png(os.path.join(self.root, self.depth[k]))
        if depth.dtype != np.uint16:
            raise RuntimeError("depth image is not 16-bit: " + self.depth[k])
        return gray, depth

    def frame_color(self, k):
        """(colour array as decoded, its pixel format, depth): RGB8 / RGBA8 [rows, cols, 3 | 4] for the device's conversion
        (vslam_rgbd_set_color_input); a grey PNG passes through as frame() returns it, with GRAY8."""
        from . import color
        img = read_png(os.path.join(self.root, self.rgb[k]))
        depth = read_png(os.path.join(self.root, self.depth[k]))
        if depth.dtype != np.uint16:
            raise RuntimeError("depth image is not 16-bit: " + self.depth[k])
        if img.ndim == 3:
            return img, (color.RGB8 if img.shape[2] == 3 else color.RGBA8), depth
        return (img if img.dtype == np.uint8 else (img >> 8).astype(np.uint8)), color.GRAY8, depth


# ---- KITTI odometry sequence folder ---------------------------------------------------------------------------------
class KittiSequence(object):
    """<root>/image_0/000000.png, <root>/image_1/000000.png, <root>/calib.txt, <root>/times.txt.  color=True: the odometry benchmark's
    colour cameras instead, <root>/image_2 and image_3 with the calibration of P2 / P3; pair(k) then returns RGB arrays [rows, cols, 3]."""

    def __init__(self, root, color=False):
        self.root = root
        self.color = bool(color)
        self.dirs = ("image_2", "image_3") if color else ("image_0", "image_1")
        self.K, self.baseline = parse_kitti_calib(os.path.join(root, "calib.txt"), (2, 3) if color else (0, 1))
        if color and not os.path.isdir(os.path.join(root, self.dirs[0])):
            raise RuntimeError("no colour cameras in this folder (image_2 / image_3): " + root)
        names = sorted(n for n in os.listdir(os.path.join(root, self.dirs[0])) if n.endswith(".png"))
        self.names = names
        tpath = os.path.join(root, "times.txt")
        self.times = [float(v) for v in open(tpath).read().split()] if os.path.exists(tpath) else list(range(len(names)))

    def __len__(self):
        return len(self.names)

    def pair(self, k):
        if self.color:
            left, right = (read_png(os.path.join(self.root, d, self.names[k])) for d in self.dirs)
            if left.ndim != 3 or right.ndim != 3 or left.dtype != np.uint8:
                raise RuntimeError("not an 8-bit colour PNG pair: " + self.names[k])
            return np.ascontiguousarray(left[:, :, :3]), np.ascontiguousarray(right[:, :, :3])
        left = read_png_gray8(os.path.join(self.root, "image_0", self.names[k]))
        right = read_png_gray8(os.path.join(self.root, "image_1", self.names[k]))
        return left, right


# ---- EuRoC / ASL folder (mav0/cam0|cam1/data.csv + data/<timestamp>.png) ----------------------------------------------------------
class EurocSequence(object):
    """`<root>/mav0/cam0/data.csv` and `cam1/data.csv` list `timestamp_ns,filename` (one `#` header line); images live in
    `camN/data/`.  Pairs are formed on equal time stamps (the two cameras are hardware-synchronised); `times` in seconds.
    Calibration: configuration_euroc.yaml's data set is rectified upstream by the message converter
    (executables/srrg_proslam_synchronizer / ROS rectification), so K / baseline come from the caller or from
    `vslam_default_config_euroc`; `calibration()` reads them from an optional `calib.txt` in KITTI P0/P1 form when a
    rectified export carries one.  Ground truth for trajectory_analyzer: `mav0/state_groundtruth_estimate0/data.csv` or
    `mav0/leica0/data.csv` (`ground_truth_path`)."""

    def __init__(self, root):
        self.root = root
        base = os.path.join(root, "mav0") if os.path.isdir(os.path.join(root, "mav0")) else root
        self.base = base
        left = self._listing(os.path.join(base, "cam0"))
        right = dict(self._listing(os.path.join(base, "cam1")))
        self.stamps, self.left, self.right = [], [], []
        for ts, name in left:
            if ts in right:
                self.stamps.append(ts); self.left.append(name); self.right.append(right[ts])
        self.times = [ts / 1e9 for ts in self.stamps]

    @staticmethod
    def _listing(cam_dir):
        path = os.path.join(cam_dir, "data.csv")
        out = []
        with open(path) as f:
            for line in f:
                line = line.strip()
                if not line or line[0] == "#":
                    continue
                a = line.split(",")
                out.append((int(a[0]), a[1].strip() if len(a) > 1 and a[1].strip() else a[0].strip() + ".png"))
        return out

    def __len__(self):
        return len(self.stamps)

    def pair(self, k):
        return (read_png_gray8(os.path.join(self.base, "cam0", "data", self.left[k])),
                read_png_gray8(os.path.join(self.base, "cam1", "data", self.right[k])))

    def calibration(self):
        path = os.path.join(self.root, "calib.txt")
        return parse_kitti_calib(path) if os.path.exists(path) else None

    def raw_calibration(self):
        """The raw rig from `mav0/cam{0,1}/sensor.yaml`: (left CameraModel, right CameraModel, R, T) with X1 = R X0 + T, the
        cam0 -> cam1 transform inv(T_BS1) T_BS0; None when the files are absent.  Feed it to rectify.rectification()."""
        from . import rectify
        paths = [os.path.join(self.base, cam, "sensor.yaml") for cam in ("cam0", "cam1")]
        if not all(os.path.exists(p) for p in paths):
            return None
        cams, T_BS = [], []
        for p in paths:
            y = read_sensor_yaml(p)
            model = str(y.get("camera_model", "pinhole"))
            if model != "pinhole":
                raise ValueError("%s: camera_model %r is not supported (pinhole only)" % (p, model))
            fu, fv, cu, cv = [float(v) for v in y["intrinsics"]]
            cols, rows = [int(v) for v in y["resolution"]]
            K = np.array([[fu, 0, cu], [0, fv, cv], [0, 0, 1]], np.float64)
            cams.append(rectify.CameraModel(K, y["distortion_coefficients"], rows, cols, str(y.get("distortion_model", "radial-tangential"))))
            T_BS.append(np.array(y["T_BS"]["data"], np.float64).reshape(4, 4))
        T10 = np.linalg.inv(T_BS[1]) @ T_BS[0]
        return cams[0], cams[1], T10[:3, :3].copy(), T10[:3, 3].copy()

    @property
    def ground_truth_path(self):
        for sub in ("state_groundtruth_estimate0", "leica0"):
            p = os.path.join(self.base, sub, "data.csv")
            if os.path.exists(p):
                return p
        return None


def _yaml_value(text):
    text = text.strip()
    if text.startswith("["):
        return [_yaml_value(v) for v in text.strip("[]").split(",") if v.strip()]
    try:
        return int(text)
    except ValueError:
        pass
    try:
        return float(text)
    except ValueError:
        return text.strip("'\"")


def read_sensor_yaml(path):
    """The keys of an ASL `sensor.yaml` this package reads (`T_BS: {rows, cols, data: [...]}`, `resolution`, `intrinsics`,
    `distortion_model`, `distortion_coefficients`, ...): `key: value` lines, one level of nesting by indentation, bracketed
    lists that may span lines, `#` comments.  Not a general YAML parser."""
    out, parent, pending = {}, None, None
    with open(path) as f:
        lines = f.read().splitlines()
    for line in lines:
        body = line.split("#", 1)[0].rstrip()
        if not body.strip() or body.strip() == "%YAML:1.0" or body.strip() == "---":
            continue
        if pending is not None:                       # continuation of a bracketed list
            target, key, acc = pending
            acc += " " + body.strip()
            if "]" in acc:
                target[key] = _yaml_value(acc)
                pending = None
            else:
                pending = (target, key, acc)
            continue
        indent = len(body) - len(body.lstrip())
        key, _, val = body.strip().partition(":")
        key, val = key.strip(), val.strip()
        if indent == 0:
            parent = None
        target = out if indent == 0 or parent is None else out[parent]
        if not val:
            if indent == 0:
                out[key] = {}
                parent = key
            continue
        if val.startswith("!!"):                        # OpenCV-style type tag (e.g. !!opencv-matrix): the mapping follows
            out[key] = {}
            parent = key
            continue
        if val.startswith("[") and "]" not in val:
            pending = (target, key, val)
            continue
        target[key] = _yaml_value(val)
    return out


# ---- trajectory writers -----------------------------------------------------------------------------------------------
PLY_INT_FIELDS = ("id", "first_frame", "last_frame", "updates")
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def write_ply(path, xyz, rgb=None, **ints):
    """Binary little-endian PLY point cloud: x y z (double) plus one int property per keyword (default: the landmark map's
    id, first_frame, last_frame, updates; missing ones are written as -1).  rgb (uint8 [n, 3]): three uchar properties red, green, blue
    behind the int properties, the names point-cloud viewers colour by; without it the file has none."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    n = xyz.shape[0]
    names = list(PLY_INT_FIELDS) + [k for k in ints if k not in PLY_INT_FIELDS]
    colours = [] if rgb is None else ["red", "green", "blue"]
    dt = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8")] + [(k, "<i4") for k in names] + [(k, "u1") for k in colours])
    rec = np.zeros(n, dt)
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    for k in names:
        rec[k] = np.asarray(ints[k], np.int32).reshape(n) if k in ints else -1
    if colours:
        c = np.asarray(rgb)
        if c.dtype != np.uint8 or c.shape != (n, 3):
            raise ValueError("write_ply: rgb must be uint8 [%d, 3], got %s %r" % (n, c.dtype, c.shape))
        for j, k in enumerate(colours):
            rec[k] = c[:, j]
    head = ["ply", "format binary_little_endian 1.0", "comment landmark map", "element vertex %d" % n,
            "property double x", "property double y", "property double z"] + ["property int %s" % k for k in names] + \
           ["property uchar %s" % k for k in colours] + ["end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        f.write(rec.tobytes())


def read_ply(path):
    """The vertex element of a binary little-endian PLY with scalar properties -> dict: xyz [n, 3] float64 and every other property
    as an array of its own type."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError("%s: not a PLY file" % path)
    body = data.index(b"\n", end) + 1
    fmt, n, props, elem = None, 0, [], None
    for line in data[:end].decode("ascii").splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elem = w[1]
            if elem == "vertex":
                n = int(w[2])
            elif props or n:
                raise ValueError("%s: only a vertex element is supported" % path)
        elif w[0] == "property" and elem == "vertex":
            if w[1] == "list" or w[1] not in _PLY_TYPES:
                raise ValueError("%s: unsupported property %r" % (path, line))
            props.append((w[2], "<" + _PLY_TYPES[w[1]]))
    if fmt != "binary_little_endian":
        raise ValueError("%s: format %s (binary_little_endian expected)" % (path, fmt))
    rec = np.frombuffer(data, np.dtype(props), count=n, offset=body)
    out = {"xyz": np.stack([rec["x"], rec["y"], rec["z"]], 1).astype(np.float64)}
    for k, _ in props:
        if k not in ("x", "y", "z"):
            out[k] = rec[k].copy()
    return out


# ---- the structure-and-motion bundle: trajectory + landmark map + observation log --------------------------------------------
BUNDLE_MAP_FIELDS = ("id", "xyz", "first_frame", "last_frame", "updates")      # always there; desc / chunk / rgb when the map has them


def write_bundle(path, K, baseline_h, poses, lm_map, obs):
    """One .npz with everything a mapping or bundle-adjustment back end needs: K [3, 3], baseline_h [3] (vslam_config: the right
    camera projects K p + baseline_h), poses [F, 12] (camera_left_to_world, row-major 3x4), the map arrays of capi.CApi.map /
    sharding.assemble_map under map_<name>, and the observation log (capi.CApi.observations / sharding.assemble_observations) as
    obs_id, obs_frame, obs_kp [n, 4] (xL, yL, xR, yR).  obs_id indexes the map arrays, obs_frame the poses.  Written to `path`
    exactly (no suffix is added); arrays keep their dtypes, so read_bundle returns them bit for bit."""
    arrays = {"K": np.asarray(K, np.float64).reshape(3, 3), "baseline_h": np.asarray(baseline_h, np.float64).reshape(3),
              "poses": np.asarray(poses, np.float64).reshape(-1, 12)}
    for k in BUNDLE_MAP_FIELDS:
        arrays["map_" + k] = np.asarray(lm_map[k])
    for k in ("desc", "chunk", "rgb"):
        if k in lm_map:
            arrays["map_" + k] = np.asarray(lm_map[k])
    arrays["obs_id"] = np.asarray(obs["id"], np.int32)
    arrays["obs_frame"] = np.asarray(obs["frame"], np.int32)
    arrays["obs_kp"] = np.asarray(obs["kp"], np.int16).reshape(-1, 4)
    with open(path, "wb") as f:
        np.savez(f, **arrays)


def read_bundle(path):
    """write_bundle's file -> dict: K, baseline_h, poses [F, 12], map (dict of the map arrays), obs_id, obs_frame, obs_kp."""
    with np.load(path) as z:
        out = {k: z[k] for k in ("K", "baseline_h", "poses", "obs_id", "obs_frame", "obs_kp")}
        out["map"] = {k[4:]: z[k] for k in z.files if k.startswith("map_")}
    return out


def write_bundle_rgbd(path, K, poses, lm_map, obs):
    """The bundle of the RGB-D tracker (capi.RgbdTracker.map / .observations): K [3, 3], poses [F, 12], the map arrays under
    map_<name>, and the log as obs_id, obs_frame, obs_xy [n, 2] float32 (the keypoint) and obs_cam [n, 3] float64 (the point's camera
    coordinates: pixel and depth measurement).  One camera, so no baseline_h and no obs_kp: read it with read_bundle_rgbd."""
    arrays = {"K": np.asarray(K, np.float64).reshape(3, 3), "poses": np.asarray(poses, np.float64).reshape(-1, 12)}
    for k in BUNDLE_MAP_FIELDS:
        arrays["map_" + k] = np.asarray(lm_map[k])
    for k in ("desc", "rgb"):
        if k in lm_map:
            arrays["map_" + k] = np.asarray(lm_map[k])
    arrays["obs_id"] = np.asarray(obs["id"], np.int32)
    arrays["obs_frame"] = np.asarray(obs["frame"], np.int32)
    arrays["obs_xy"] = np.asarray(obs["xy"], np.float32).reshape(-1, 2)
    arrays["obs_cam"] = np.asarray(obs["cam"], np.float64).reshape(-1, 3)
    with open(path, "wb") as f:
        np.savez(f, **arrays)


def read_bundle_rgbd(path):
    """write_bundle_rgbd's file -> dict: K, poses [F, 12], map (dict of the map arrays), obs_id, obs_frame, obs_xy, obs_cam."""
    with np.load(path) as z:
        out = {k: z[k] for k in ("K", "poses", "obs_id", "obs_frame", "obs_xy", "obs_cam")}
        out["map"] = {k[4:]: z[k] for k in z.files if k.startswith("map_")}
    return out


def write_observations_text(path, obs_id, obs_frame, obs_kp):
    """One observation per line, `frame id xL yL xR yR`, in the log's order (by frame, then by point order)."""
    kp = np.asarray(obs_kp).reshape(-1, 4)
    with open(path, "w") as f:
        for i, fr, k in zip(np.asarray(obs_id).tolist(), np.asarray(obs_frame).tolist(), kp.tolist()):
            f.write("%d %d %d %d %d %d\n" % (fr, i, k[0], k[1], k[2], k[3]))


def write_trajectory_kitti(path, poses):
    with open(path, "w") as f:
        for T in np.asarray(poses, np.float64).reshape(-1, 12):
            f.write("".join("%.9f " % v for v in T) + "\n")


def rotation_to_quaternion(R):
    """Eigen::Quaternion(Matrix3) (xyzw returned)."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = R[0, 0] + R[1, 1] + R[2, 2]
    if t > 0:
        t = np.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        x, y, z = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q = [0.0, 0.0, 0.0]
        q[i] = 0.5 * t
        t = 0.5 / t
        w = (R[k, j] - R[j, k]) * t
        q[j] = (R[j, i] + R[i, j]) * t
        q[k] = (R[k, i] + R[i, k]) * t
        x, y, z = q
    return x, y, z, w


def write_trajectory_tum(path, poses, timestamps):
    with open(path, "w") as f:
        for T, ts in zip(np.asarray(poses, np.float64).reshape(-1, 3, 4), timestamps):
            x, y, z, w = rotation_to_quaternion(T[:, :3])
            vals = (ts, T[0, 3], T[1, 3], T[2, 3], x, y, z, w)
            f.write("".join("%.9f " % v for v in vals) + "\n")


def read_trajectory_kitti(path):
    return np.loadtxt(path).reshape(-1, 3, 4)


def quaternion_to_rotation(x, y, z, w):
    """Eigen::Quaternion::toRotationMatrix of the normalised quaternion."""
    n = np.sqrt(x * x + y * y + z * z + w * w)
    x, y, z, w = x / n, y / n, z / n, w / n
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float64)


def read_trajectory_tum(path):
    """`timestamp tx ty tz qx qy qz qw` lines (`#` comments): (timestamps float64 [n], poses float64 [n, 3, 4])."""
    rows = read_tum_list(path)
    times = np.array([t for t, _ in rows], np.float64)
    poses = np.zeros((len(rows), 3, 4), np.float64)
    for k, (_, a) in enumerate(rows):
        if len(a) != 7:
            raise ValueError("%s: line %d has %d values behind the time stamp, a TUM trajectory has 7" % (path, k + 1, len(a)))
        v = [float(s) for s in a]
        poses[k, :, :3] = quaternion_to_rotation(*v[3:])
        poses[k, :, 3] = v[:3]
    return times, poses


def read_pose_guesses(path, frame_times, max_difference=0.02):
    """An odometry file for the frames of a sequence: float64 [n_frames, 12] camera_left_to_world and bool [n_frames] (the frame has a
    pose of its own).  A KITTI pose file (12 values per line) is taken line k for frame k; a TUM trajectory (8 values) is associated to
    the frames' time stamps like rgb.txt to depth.txt (associate: nearest first, within max_difference seconds).  A frame without a pose
    carries the last one before it (identity ahead of the first), as a tracker that is handed no new guess re-uses the last."""
    n = len(frame_times)
    with open(path) as f:
        first = next((ln for ln in f if ln.strip() and ln.strip()[0] != "#"), "")
    width = len(first.replace(",", " ").split())
    own = np.zeros(n, bool)
    out = np.zeros((n, 12), np.float64)
    if width == 12:
        poses = read_trajectory_kitti(path).reshape(-1, 12)
        m = min(n, len(poses))
        out[:m], own[:m] = poses[:m], True
    elif width == 8:
        times, poses = read_trajectory_tum(path)
        for i, j in associate(list(np.asarray(frame_times, np.float64)), list(times), max_difference):
            out[i], own[i] = poses[j].reshape(12), True
    else:
        raise ValueError("%s: %d values per line (a KITTI pose file has 12, a TUM trajectory 8)" % (path, width))
    last = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)
    for k in range(n):
        if own[k]:
            last = out[k]
        else:
            out[k] = last
    return out, own

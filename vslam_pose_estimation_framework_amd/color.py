"""Interleaved 8-bit colour to grey, restated in numpy: the one definition of the project,

    gray = (R * 4899 + G * 9617 + B * 1868 + 8192) >> 14        all integer; alpha is ignored

[recalled: cvtColor on 8-bit images with 14 fractional bits, the OpenCV 3.x of the reference's image; io_formats.rgb_to_gray_opencv states
the same for RGB arrays].  Newer OpenCV uses 15 bits (9798 / 19235 / 3735): not built.

The reference of the tests of the device path (kernels_gray.h: vslam_set_color_input, vslam_rgbd_set_color_input, vslam_gray_u8) and a host
fallback for callers without a device."""
import numpy as np

GRAY8, BGR8, RGB8, BGRA8, RGBA8 = 0, 1, 2, 3, 4      # VSLAM_PIXEL_* of include/vslam_hip.h
FORMATS = (BGR8, RGB8, BGRA8, RGBA8)
NAMES = {GRAY8: "gray8", BGR8: "bgr8", RGB8: "rgb8", BGRA8: "bgra8", RGBA8: "rgba8"}
CR, CG, CB, SHIFT = 4899, 9617, 1868, 14


def channels(fmt):
    """Bytes per pixel of a format."""
    if fmt == GRAY8:
        return 1
    if fmt in (BGR8, RGB8):
        return 3
    if fmt in (BGRA8, RGBA8):
        return 4
    raise ValueError("unknown pixel format %r" % (fmt,))


def to_gray_u8(image, fmt):
    """image: uint8 [..., channels(fmt)] (a GRAY8 image: [...], returned as it is) -> uint8 [...]."""
    img = np.asarray(image)
    if img.dtype != np.uint8:
        raise ValueError("to_gray_u8: a uint8 image is required")
    if fmt == GRAY8:
        return img
    ch = channels(fmt)
    if img.ndim < 1 or img.shape[-1] != ch:
        raise ValueError("to_gray_u8: %s needs %d channels, the array has shape %r" % (NAMES[fmt], ch, img.shape))
    v = img.astype(np.int32)
    r, b = (v[..., 0], v[..., 2]) if fmt in (RGB8, RGBA8) else (v[..., 2], v[..., 0])
    return ((r * CR + v[..., 1] * CG + b * CB + (1 << (SHIFT - 1))) >> SHIFT).astype(np.uint8)

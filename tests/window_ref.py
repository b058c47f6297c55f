"""The intensity-window arithmetic of include/mi_unet.h restated in numpy for test_window_cpu.py and
test_gpu_window.py: np.sort for the window, an operation-by-operation fp64 restatement of the bilinear sum and the quantisation for the
bytes.  numpy rounds every operation once and never contracts, which is the contract of the kernels and of the host facade."""
import functools

import numpy as np


def ref_window(plane, clip_lo_ppm=0, clip_hi_ppm=0):
    """(lo, hi) of a u16 plane: s[k_lo], s[n - 1 - k_hi] of the sorted samples, k = floor(n * ppm / 1e6) in integers"""
    s = np.sort(np.asarray(plane, np.uint16).reshape(-1))
    n = int(s.size)
    k_lo, k_hi = n * int(clip_lo_ppm) // 1000000, n * int(clip_hi_ppm) // 1000000
    assert k_lo + k_hi <= n - 1
    return int(s[k_lo]), int(s[n - 1 - k_hi])


def ref_quantise(v, lo, hi):
    """v float64 (samples or interpolants) -> bytes under the window lo..hi"""
    L = int(lo)
    Hh = int(hi) if hi > lo else L + 1
    vc = np.minimum(np.maximum(v, np.float64(L)), np.float64(Hh))
    q = (vc - np.float64(L)) * (np.float64(255.0) / np.float64(Hh - L)) + np.float64(0.5)
    return q.astype(np.int32).astype(np.uint8)


def ref_interpolant(plane, out_w, out_h):
    """the fp64 top-left aligned bilinear interpolant of resample_u8_kernel: [out_h][out_w] float64"""
    r = np.asarray(plane, np.uint16).astype(np.float64)
    h, w = r.shape
    step_x, step_y = np.float64(w) / np.float64(out_w), np.float64(h) / np.float64(out_h)
    fx, fy = np.arange(out_w, dtype=np.float64) * step_x, np.arange(out_h, dtype=np.float64) * step_y
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    ix1, iy1 = np.minimum(ix + 1, w - 1), np.minimum(iy + 1, h - 1)
    dx, dy = (fx - ix)[None, :], (fy - iy)[:, None]
    omdx, omdy = 1.0 - dx, 1.0 - dy
    v = (omdx * omdy) * r[iy][:, ix]
    v = v + (dx * omdy) * r[iy][:, ix1]
    v = v + (omdx * dy) * r[iy1][:, ix]
    v = v + (dx * dy) * r[iy1][:, ix1]
    return v


def ref_resample(plane, lo, hi, out_w, out_h):
    """the tile of the resampling path under the window lo..hi: u8 [out_h][out_w]"""
    return ref_quantise(ref_interpolant(plane, out_w, out_h), lo, hi)


def ref_normalise(plane, lo, hi):
    """the tiled path: no resampling, the sample itself"""
    return ref_quantise(np.asarray(plane, np.uint16).astype(np.float64), lo, hi)


@functools.lru_cache(maxsize=None)
def nine_planes():
    """The smallest planes that reach every branch of the selection: shorter than one 16-byte vector (1 x 1, 1 x 7), ragged tails
    (3 x 5; 1031 x 517 = 533027 samples, 3 past the last vector, 66 workgroups), several workgroups with both ranks under one high
    byte (512 x 512 inside 0x0B00 .. 0x0BFF), ranks under different high bytes (values over 0 .. 65535), a constant plane, one hot
    and one dead pixel on ~N(3000, 400), and all 65535 (the u16 wrap of the min/max path).  Nine images = micro-batches 4, 4, 1."""
    rng = np.random.default_rng(20250117)
    hot = np.clip(rng.normal(3000.0, 400.0, (300, 400)), 1, 65534).astype(np.uint16)
    hot[17, 23], hot[211, 305] = 65535, 0
    planes = [
        rng.integers(0, 65536, (1, 1)),
        rng.integers(0, 65536, (1, 7)),
        rng.integers(0, 65536, (3, 5)),
        np.clip(rng.normal(3000.0, 400.0, (1031, 517)), 0, 65535),
        rng.integers(0x0B05, 0x0BFB, (512, 512)),
        rng.integers(0, 65536, (200, 300)),
        np.full((40, 50), 1234),
        hot,
        np.full((16, 16), 65535),
    ]
    return tuple(np.ascontiguousarray(p, dtype=np.uint16) for p in planes)


HOT = 7       # index of the hot-and-dead-pixel plane in nine_planes()
WRAP = 8      # ... of the all-65535 plane
SPREAD = 5    # ... of the plane whose ranks fall under different high bytes

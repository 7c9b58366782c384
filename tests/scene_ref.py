"""numpy restatements of the two scan kernels' contracts (include/ptt_hip.h, ptt_scan_ingest_f32 / ptt_scan_preload_f32), written
out operation by operation: numpy rounds every product and every sum on its own, which is the contract (no fused multiply-add),
and every step's result is stored as float32 before the next one reads it.

    ingest_ref(raw, steps)          (N, C) float32 rows -> (3, N) float32 planar, through [('rotate', 3x3) | ('translate', 3) |
                                    ('affine', 3x4 or 4x4: the top three rows)] in order
    preload_ref(points, lo, hi)     (3, N) float32 -> the columns with lo < p < hi on every axis (float32 point against float64
                                    bound, strict), in their order, values unchanged

tests/golden/make_golden_g26.py checks both against the reference's own PointCloud / crop_pc bit for bit before it writes fixture
g26; the tests compare the kernels with these.
"""
import numpy as np


def ingest_ref(raw, steps=()):
    raw = np.asarray(raw)
    assert raw.dtype == np.float32 and raw.ndim == 2 and raw.shape[1] >= 3
    p = np.ascontiguousarray(raw[:, :3].T)                              # float32 (3, N)
    for kind, m in (steps or ()):
        m = np.asarray(m, np.float64)
        x, y, z = (p[r].astype(np.float64) for r in range(3))
        q = np.empty_like(p)
        for r in range(3):
            if kind == 'rotate':
                v = (m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z
            elif kind == 'translate':
                v = (x, y, z)[r] + m[r]
            elif kind == 'affine':
                v = ((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3]
            else:
                raise ValueError(kind)
            q[r] = v.astype(np.float32)                                 # each step is stored back as float32
        p = q
    return p


def preload_ref(points, lo, hi):
    points = np.asarray(points)
    assert points.dtype == np.float32 and points.shape[0] == 3
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    keep = np.ones(points.shape[1], bool)
    for r in range(3):
        v = points[r].astype(np.float64)
        keep &= (v > lo[r]) & (v < hi[r])
    return np.ascontiguousarray(points[:, keep])


def crop_bounds(center, wlh, quat, offset):
    """lo, hi of crop_pc(pc, box, offset=offset) at scale 1.0 (kitti_tracking_utils.py:276-279), from the repo's box_math."""
    from ptt_amd.datasets.kitti import box_math as bm
    c = bm.corners(np.asarray(center, np.float64), np.asarray(wlh, np.float64) * 1.0, bm.q_rotation_matrix(np.asarray(quat, np.float64)))
    return np.min(c, 1) - offset, np.max(c, 1) + offset

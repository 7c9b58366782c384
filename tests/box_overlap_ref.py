"""TEST INFRASTRUCTURE — the reference's tracking metrics (tools/eval_utils/eval_tracking_metrics.py:37-154) restated in float64
numpy: the checker of ptt_box_overlap_f64 / ptt_amd.eval_metrics (tests/test_eval_metrics_gpu.py), itself pinned by closed-form
cases and by an independent half-space method (tests/test_eval_metrics_cpu.py).

The reference intersects the two footprints with shapely, which is not a dependency of this repository; in its place the convex
quadrilateral of one box is clipped by the four half-planes of the other (Sutherland-Hodgman) and the area taken by the shoelace
sum. Everything else is the reference's own arithmetic, quirks included: the asymmetric np.allclose of Box.__eq__
(ptt/datasets/kitti/kitti_tracking_utils.py:84-93), the height terms formed from component 1 of the centres under both coordinate
conventions (:65-67), `>=` for Success and `<=` for Precision.

A box is a row of 10 float64: centre (3), wlh (3), quaternion (w, x, y, z). Nothing here imports ptt_amd.
"""
import numpy as np

trapz = getattr(np, "trapezoid", None) or np.trapz            # np.trapz, by the name numpy 2 gives it

_SX = np.array([1, 1, 1, 1, -1, -1, -1, -1], np.float64)
_SY = np.array([1, -1, -1, 1, 1, -1, -1, 1], np.float64)
_SZ = np.array([1, 1, -1, -1, 1, 1, -1, -1], np.float64)


def box_row(center, wlh, quat):
    return np.concatenate([np.asarray(center, np.float64), np.asarray(wlh, np.float64), np.asarray(quat, np.float64)])


def q_mul(a, b):
    """Hamilton product of (w, x, y, z) quaternions."""
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def q_axis(axis, angle):
    v = np.zeros(3)
    v[axis] = 1.0
    return np.concatenate([[np.cos(angle / 2.0)], np.sin(angle / 2.0) * v])


def q_camera(ry):
    """What a KITTI label's box carries in the camera frame: q_y(ry) * q_x(pi / 2) (kitti_dataset_tracking.py:321-322)."""
    return q_mul(q_axis(1, ry), q_axis(0, np.pi / 2))


def q_lidar(yaw):
    return q_axis(2, yaw)


def rotation_matrix(q):
    """Quaternion.rotation_matrix: of the normalised quaternion (left alone when unit to 1e-14, as pyquaternion does)."""
    q = np.asarray(q, np.float64)
    n = np.sqrt(np.dot(q, q))
    if not abs(1.0 - n * n) < 1e-14 and n > 0:
        q = q / n
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def corners(box):
    """Box.corners (kitti_tracking_utils.py:132-150) -> (3, 8)."""
    w, l, h = box[3:6]
    local = np.vstack((l / 2 * _SX, w / 2 * _SY, h / 2 * _SZ))
    return np.dot(rotation_matrix(box[6:10]), local) + box[0:3, None]


def footprint(box, ref_coord):
    """fromBoxToPoly (:45-49) -> (4, 2) vertices."""
    k = corners(box)
    coord = ref_coord.lower()
    if coord == 'camera':
        return k[[0, 2]].T[[0, 1, 5, 4]]
    if coord == 'lidar':
        return k[:, [2, 3, 7, 6]][0:2].T                                # bottom_corners(), which shapely reads as (x, y)
    raise ValueError(ref_coord)


def signed_area(poly):
    x, y = poly[:, 0], poly[:, 1]
    return 0.5 * np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y)


def clip_area(subject, clip):
    """Area of the intersection of two convex polygons: `subject` through the half-planes of `clip` (Sutherland-Hodgman), both
    put in counter-clockwise order first; fewer than 3 vertices left = 0."""
    if signed_area(subject) < 0:
        subject = subject[::-1]
    if signed_area(clip) < 0:
        clip = clip[::-1]
    out = [(float(p[0]), float(p[1])) for p in subject]
    n = len(clip)
    for i in range(n):
        a, b = clip[i], clip[(i + 1) % n]
        inp, out = out, []
        if not inp:
            break
        ex, ey = b[0] - a[0], b[1] - a[1]
        for j in range(len(inp)):
            p, q = inp[j], inp[(j + 1) % len(inp)]
            sp = ex * (p[1] - a[1]) - ey * (p[0] - a[0])
            sq = ex * (q[1] - a[1]) - ey * (q[0] - a[0])
            if sp >= 0:
                out.append(p)
            if (sp >= 0) != (sq >= 0):
                t = sp / (sp - sq)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
    return abs(signed_area(np.array(out))) if len(out) >= 3 else 0.0


def boxes_equal(box_a, box_b):
    """Box.__eq__ (:84-93) on what a box carries here (no label, score or velocity): np.allclose with numpy's defaults,
    |a - b| <= 1e-8 + 1e-5 * |b|."""
    return bool(np.allclose(box_a[0:3], box_b[0:3]) and np.allclose(box_a[3:6], box_b[3:6]) and np.allclose(box_a[6:10], box_b[6:10]))


def intersection_area(box_a, box_b, ref_coord):
    return clip_area(footprint(box_a, ref_coord), footprint(box_b, ref_coord))


def estimateAccuracy(box_a, box_b, dim=3):
    if dim == 3:
        return float(np.linalg.norm(box_a[0:3] - box_b[0:3], ord=2))
    elif dim == 2:
        return float(np.linalg.norm(box_a[[0, 2]] - box_b[[0, 2]], ord=2))
    raise ValueError(dim)


def estimateOverlap(box_a, box_b, dim=2, ref_coord='camera'):
    if boxes_equal(box_a, box_b):
        return 1.0
    poly_anno, poly_subm = footprint(box_a, ref_coord), footprint(box_b, ref_coord)
    inter = clip_area(poly_anno, poly_subm)
    if dim == 2:
        union = abs(signed_area(poly_anno)) + abs(signed_area(poly_subm)) - inter
        return float(inter / union)
    ymax = min(box_a[1], box_b[1])
    ymin = max(box_a[1] - box_a[5], box_b[1] - box_b[5])
    inter_vol = inter * max(0, ymax - ymin)
    anno_vol = box_a[3] * box_a[4] * box_a[5]
    subm_vol = box_b[3] * box_b[4] * box_b[5]
    return float(inter_vol * 1.0 / (anno_vol + subm_vol - inter_vol))


def overlaps(gt, pred, ref_coord, dim=3):
    """(n, 10), (n, 10) -> overlap (n,), accuracy (n,): one estimateOverlap / estimateAccuracy per row."""
    gt, pred = np.asarray(gt, np.float64).reshape(-1, 10), np.asarray(pred, np.float64).reshape(-1, 10)
    ov = np.array([estimateOverlap(a, b, dim, ref_coord) for a, b in zip(gt, pred)], np.float64)
    acc = np.array([estimateAccuracy(a, b, dim) for a, b in zip(gt, pred)], np.float64)
    return ov, acc


class Success(object):
    """:77-113, one comparison at a time as the reference makes them."""

    def __init__(self, n=21, max_overlap=1):
        self.max_overlap = max_overlap
        self.Xaxis = np.linspace(0, self.max_overlap, n)
        self.overlaps = []

    def add_overlap(self, val):
        self.overlaps.append(val)

    @property
    def count(self):
        return len(self.overlaps)

    @property
    def counts(self):
        return np.array([sum(1 for i in self.overlaps if i >= thres) for thres in self.Xaxis])

    @property
    def value(self):
        return self.counts.astype(float) / self.count

    @property
    def average(self):
        if len(self.overlaps) == 0:
            return 0
        return trapz(self.value, x=self.Xaxis) * 100 / self.max_overlap


class Precision(object):
    """:116-154."""

    def __init__(self, n=21, max_accuracy=2):
        self.max_accuracy = max_accuracy
        self.Xaxis = np.linspace(0, self.max_accuracy, n)
        self.accuracies = []

    def add_accuracy(self, val):
        self.accuracies.append(val)

    @property
    def count(self):
        return len(self.accuracies)

    @property
    def counts(self):
        return np.array([sum(1 for i in self.accuracies if i <= thres) for thres in self.Xaxis])

    @property
    def value(self):
        return self.counts.astype(float) / self.count

    @property
    def average(self):
        if len(self.accuracies) == 0:
            return 0
        return trapz(self.value, x=self.Xaxis) * 100 / self.max_accuracy


def halfspace_area(poly_a, poly_b):
    """The same intersection area by an independent method: the eight half-planes of the two quadrilaterals handed to
    scipy.spatial.HalfspaceIntersection (an interior point from a linear programme), the area from ConvexHull. None when the
    intersection has no interior to speak of (inscribed radius < 1e-9)."""
    from scipy.optimize import linprog
    from scipy.spatial import ConvexHull, HalfspaceIntersection
    hs = []
    for p in (poly_a, poly_b):
        if signed_area(p) < 0:
            p = p[::-1]
        for i in range(4):
            a, b = p[i], p[(i + 1) % 4]
            nrm = np.array([b[1] - a[1], -(b[0] - a[0])])               # outward normal of a counter-clockwise edge
            hs.append([nrm[0], nrm[1], -np.dot(nrm, a)])
    hs = np.array(hs)
    norms = np.linalg.norm(hs[:, :2], axis=1)
    r = linprog([0, 0, -1], A_ub=np.c_[hs[:, :2], norms], b_ub=-hs[:, 2], bounds=[(None, None)] * 2 + [(0, None)])
    if r.status != 0 or r.x[2] < 1e-9:
        return None
    return float(ConvexHull(HalfspaceIntersection(hs, r.x[:2]).intersections).volume)


def random_pairs(seed, n, ref_coord):
    """The seeded random set of the tests: a box with its centre within +-40 m, any yaw, car-to-van sizes; its partner with the
    centre off by N(0, 0.6 m), the yaw by N(0, 0.3 rad) and the sizes scaled by U(0.8, 1.2). -> gt (n, 10), pred (n, 10)."""
    rs = np.random.RandomState(seed)
    quat = q_camera if ref_coord.lower() == 'camera' else q_lidar
    gt, pred = np.empty((n, 10)), np.empty((n, 10))
    for i in range(n):
        c = rs.uniform(-39.0, 39.0, 3)
        wlh = rs.uniform([0.4, 0.4, 0.8], [2.2, 5.0, 2.2])
        ang = rs.uniform(-np.pi, np.pi)
        c2 = np.clip(c + rs.normal(0, 0.6, 3), -40.0, 40.0)
        gt[i] = box_row(c, wlh, quat(ang))
        pred[i] = box_row(c2, wlh * rs.uniform(0.8, 1.2, 3), quat(ang + rs.normal(0, 0.3)))
    return gt, pred

"""A small synthetic KITTI tracking directory, written from a seed: what tests/golden/make_golden_g28.py runs the reference's
KittiTrackingDataset on and what the kitti tests read — the same bytes in both, so the tree itself is not committed.

    root/training/velodyne/<scene>/<frame:06d>.bin     (N, 4) float32, 300..500 points
                  label_02/<scene>.txt                 17 columns, six decimals as KITTI writes them
                  calib/<scene>.txt                    P0..P3 (keys with a colon), R_rect, Tr_velo_cam, Tr_imu_velo

Scenes 0000, 0019, 0020 of FRAMES frames. Per scene: Car track 0 over frames 1..4, Car track 1 over frames 0..3, Pedestrian
track 2 over all frames, and a DontCare row (track_id -1) per frame. Objects are made in the velodyne frame — a cluster of
points inside a moving box, over scattered background — and annotated through R_rect . Tr_velo_cam, a rigid transform a few
hundredths of a radian off KITTI's axis permutation, with a non-identity R_rect. MISSING = ('0020', 2) is annotated but has no
.bin. The last row of Car track 1 in scene 0019 (LINE_ROW) carries rotation_y = -pi/2 to full precision: under REF_COOR lidar
its box has the identity orientation, so its corners are sums of one rounding each whatever the order of evaluation (the
result-line test compares characters).
"""
import os

import numpy as np

SCENES = ("0000", "0019", "0020")
FRAMES = 5
MISSING = ("0020", 2)
CAR_POINTS, PED_POINTS = 60, 40
TRACKS = ((0, "Car", 1, 5), (1, "Car", 0, 4), (2, "Pedestrian", 0, 5))          # (track_id, type, first frame, end)
LINE_ROW = ("0019", 1, 3)                                                        # (scene, track_id, frame)


def _rot(axis_angle):
    """Rodrigues' formula."""
    v = np.asarray(axis_angle, np.float64)
    t = np.linalg.norm(v)
    if t == 0:
        return np.eye(3)
    k = v / t
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def _fmt(values):
    return " ".join("%.12e" % v for v in np.asarray(values, np.float64).reshape(-1))


def write_tree(root, seed):
    """Writes the tree under `root` (created if need be). -> {'scenes', 'missing', 'line_row'}."""
    rs = np.random.RandomState(seed)
    base = os.path.join(str(root), "training")
    for sub in ("velodyne", "label_02", "calib"):
        os.makedirs(os.path.join(base, sub), exist_ok=True)
    permute = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])     # velodyne (front, left, up) -> camera (right, down, front)
    for scene in SCENES:
        os.makedirs(os.path.join(base, "velodyne", scene), exist_ok=True)
        R = _rot(rs.uniform(-0.02, 0.02, 3)) @ permute
        t = np.array([-0.004, -0.072, -0.268]) + rs.uniform(-0.01, 0.01, 3)
        R0 = _rot(rs.uniform(-0.004, 0.004, 3))
        P2 = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])
        with open(os.path.join(base, "calib", scene + ".txt"), "w") as f:
            for k in range(4):
                f.write("P%d: %s\n" % (k, _fmt(P2)))
            f.write("R_rect %s\n" % _fmt(R0))
            f.write("Tr_velo_cam %s\n" % _fmt(np.hstack([R, t[:, None]])))
            f.write("Tr_imu_velo %s\n" % _fmt(np.hstack([np.eye(3), [[-0.81], [0.32], [-0.8]]])))
        # the objects, in the velodyne frame: start, heading, speed, size (w, l, h)
        objs = {}
        for track_id, kind, first, end in TRACKS:
            car = kind == "Car"
            objs[track_id] = dict(start=np.array([rs.uniform(6, 9) + 4.0 * track_id, rs.uniform(-5, 5), 0.0]), yaw=rs.uniform(-np.pi, np.pi),
                                  speed=rs.uniform(0.2, 0.6), turn=rs.uniform(-0.05, 0.05),
                                  wlh=np.array([rs.uniform(1.6, 1.9), rs.uniform(3.8, 4.5), rs.uniform(1.4, 1.6)]) if car
                                  else np.array([rs.uniform(0.5, 0.7), rs.uniform(0.6, 0.9), rs.uniform(1.6, 1.8)]))
        lines = []
        for frame in range(FRAMES):
            clouds = [rs.uniform(-1, 1, (rs.randint(150, 291), 3)) * [30.0, 30.0, 1.5] + [10.0, 0.0, 0.0]]
            for track_id, kind, first, end in TRACKS:
                o = objs[track_id]
                yaw = o["yaw"] + o["turn"] * frame
                if (scene, track_id, frame) == LINE_ROW:
                    yaw = 0.0
                w, l, h = o["wlh"]
                center = o["start"] + o["speed"] * frame * np.array([np.cos(o["yaw"]), np.sin(o["yaw"]), 0.0]) + [0.0, 0.0, h / 2 - 1.7]
                n = CAR_POINTS if kind == "Car" else PED_POINTS
                local = rs.uniform(-0.42, 0.42, (n, 3)) * [l, w, h]              # length along the heading
                clouds.append(local @ _rot([0.0, 0.0, yaw]).T + center)          # the object is scanned whether or not it is annotated
                if not first <= frame < end:
                    continue
                bottom = center - [0.0, 0.0, h / 2]
                x, y, z = R0 @ (R @ bottom + t)
                ry = repr(-np.pi / 2) if (scene, track_id, frame) == LINE_ROW else "%.6f" % (-(yaw + np.pi / 2))
                lines.append("%d %d %s 0 0 %.6f %.6f %.6f %.6f %.6f %.6f %.6f %.6f %.6f %.6f %.6f %s"
                             % (frame, track_id, kind, rs.uniform(-3, 3), 100.0 + track_id, 150.0, 200.0 + track_id, 250.0, h, w, l, x, y, z, ry))
            lines.append("%d -1 DontCare -1 -1 -10.000000 %.6f %.6f %.6f %.6f -1000.000000 -1000.000000 -1000.000000 -10.000000 -1 -1 -1"
                         % (frame, rs.uniform(0, 300), rs.uniform(0, 100), rs.uniform(300, 600), rs.uniform(100, 300)))
            pts = np.concatenate(clouds, 0)
            raw = np.concatenate([pts[rs.permutation(len(pts))], rs.uniform(0, 1, (len(pts), 1))], 1).astype(np.float32)
            assert 300 <= len(raw) <= 500
            if (scene, frame) != MISSING:
                np.ascontiguousarray(raw).tofile(os.path.join(base, "velodyne", scene, "%06d.bin" % frame))
        with open(os.path.join(base, "label_02", scene + ".txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    return {"scenes": SCENES, "missing": MISSING, "line_row": LINE_ROW}

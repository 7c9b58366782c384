"""numpy statement of feature-space furthest point sampling (sample_method 'ffps'), the definition in include/ptt_hip.h under
ptt_ffps_f32. A plain module: no device, no fixtures.

    ffps(xyz, feat, npoint)        the definition: v_k = [xyz_k ; feat_k], d(i,k) a float32 accumulator over c = 0 .. D-1 in order,
                                   every operation a float32 numpy elementwise operation (one rounding each, nothing fused)
    fps_with_dist(D, npoint)       the same loop on a given (B,N,N) matrix: what _ext.furthest_point_sampling_with_dist would do
                                   (pointnet2_utils.py:27-55); np.argmax returns the lowest index among equal maxima
"""
import numpy as np


def fps_with_dist(D, npoint):
    """D (B,N,N) -> (B,npoint) int32: tmp = 1e10, idx[0] = 0, tmp = min(tmp, D[last]), idx[j] = argmax tmp (lowest index)."""
    D = np.asarray(D, np.float32)
    B, N, _ = D.shape
    out = np.zeros((B, npoint), np.int32)
    for b in range(B):
        tmp = np.full((N,), 1e10, np.float32)
        last = 0
        for j in range(1, npoint):
            tmp = np.minimum(tmp, D[b, last])
            last = int(np.argmax(tmp))
            out[b, j] = last
    return out


def dist_row(v, i):
    """v (N,D) float32 -> d(i, :) (N,) float32: acc = 0; for c in order: t = v[i,c] - v[:,c]; acc = acc + t*t."""
    acc = np.zeros((v.shape[0],), np.float32)
    for c in range(v.shape[1]):
        t = v[i, c] - v[:, c]
        acc = acc + t * t
    return acc


def ffps(xyz, feat, npoint):
    """xyz (B,N,3), feat (B,C,N) or None -> (B,npoint) int32."""
    xyz = np.asarray(xyz, np.float32)
    B, N, _ = xyz.shape
    out = np.zeros((B, npoint), np.int32)
    for b in range(B):
        v = xyz[b] if feat is None else np.concatenate([xyz[b], np.asarray(feat[b], np.float32).T], axis=1)
        v = np.ascontiguousarray(v, np.float32)
        tmp = np.full((N,), 1e10, np.float32)
        last = 0
        for j in range(1, npoint):
            tmp = np.minimum(tmp, dist_row(v, last))
            last = int(np.argmax(tmp))
            out[b, j] = last
    return out


def exact_cloud(rs, B, N, C):
    """Values that are multiples of 1/4 in [-4, 4]: every product and every partial sum of a distance over up to a few hundred
    channels is a multiple of 1/16 below 2^24 / 16, exact in float32 in ANY summation order -> (xyz (B,N,3), feat (B,C,N))."""
    q = lambda shape: (rs.randint(-16, 17, shape) / 4.0).astype(np.float32)
    return q((B, N, 3)), q((B, C, N))

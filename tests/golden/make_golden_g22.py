"""Fixture G22 — the reference's OWN PointnetSAModuleVotes(sample_method='ffps') (pointnet2_modules.py:57-90), a branch its
extension could never run: `_ext.furthest_point_sampling_with_dist` does not exist upstream. Here it is stubbed, like the other
index ops in make_golden.py, by the numpy loop tests/ffps_ref.fps_with_dist (tmp = 1e10, idx[0] = 0, min-update, np.argmax = lowest
index), so everything AROUND the sampler is the imported reference: the concatenation order of `features_for_fps` ([xyz ; features]),
that the distance is taken on the level's INPUT features, square_distance itself, and what the chosen indices feed.

Input is exact arithmetic (multiples of 1/4 in [-4, 4]): every partial sum of a distance is exact in float32, so torch's
unspecified summation order cannot change the matrix, and a sampler with ANY fixed summation order must reproduce `inds` exactly.
B = 2, N = 64, C = 8, npoint = 32. Only arrays are committed.

    python tests/golden/make_golden_g22.py        # writes tests/golden/G22_ffps_module.npz and prints its report line
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import ffps_ref                          # noqa: E402
from tests.golden import make_golden as MG          # noqa: E402
from tests.util import mlp_layers                   # noqa: E402

B, N, C, NPOINT, RADIUS, NSAMPLE, SEED = 2, 64, 8, 32, 2.0, 16, 2222
SPEC = [C + 3, 32, 32, 64]


def main():
    MG._install_stubs()
    received = []

    def with_dist(dist, npoint):
        received.append(dist.detach().numpy().copy())
        return torch.from_numpy(ffps_ref.fps_with_dist(received[-1], npoint))

    sys.modules["pointnet2_ops._ext"].furthest_point_sampling_with_dist = with_dist
    sys.path.insert(0, MG.REF)                   # `ptt` = the reference's package
    from ptt.models.backbones_3d.pointnet2 import pointnet2_modules as ref_mod

    xyz, feat = ffps_ref.exact_cloud(np.random.RandomState(SEED), B, N, C)
    layers = mlp_layers(SEED, SPEC)
    sa = ref_mod.PointnetSAModuleVotes(mlp=[C] + SPEC[1:], radius=RADIUS, nsample=NSAMPLE, normalize_xyz=True,
                                       sample_method='ffps').eval()
    MG._load_mlp(sa.mlp_module, layers)
    with torch.no_grad():
        new_xyz, new_features, inds = sa(torch.from_numpy(xyz), torch.from_numpy(feat), NPOINT)
    assert len(received) == 1 and received[0].shape == (B, N, N) and received[0].dtype == np.float32
    assert inds.dtype == torch.int64
    # the matrix-free definition agrees with what the reference's matrix gave (asserted here; tests hold it to the arrays)
    mine = ffps_ref.ffps(xyz, feat, NPOINT)
    assert np.array_equal(mine, inds.numpy()), "ffps_ref.ffps != the reference module's picks"
    for b in range(B):
        assert len(set(mine[b].tolist())) == NPOINT
    out = {"xyz": xyz, "feats": feat, "dist": received[0], "inds": inds.numpy(), "new_xyz": new_xyz.numpy(),
           "new_features": new_features.numpy(), "radius": np.float64(RADIUS), "nsample": np.int64(NSAMPLE),
           "npoint": np.int64(NPOINT), "spec": np.array(SPEC), "seed": np.int64(SEED)}
    for li, L in enumerate(layers):
        for k, v in L.items():
            out["layer%d_%s" % (li, k)] = v.numpy() if isinstance(v, torch.Tensor) else np.float64(v)
    np.savez_compressed(os.path.join(HERE, "G22_ffps_module.npz"), **out)
    line = ("G22 PointnetSAModuleVotes(sample_method='ffps') of the reference with furthest_point_sampling_with_dist stubbed by the numpy "
            "matrix loop: exact-arithmetic input B=%d N=%d C=%d npoint=%d; matrix-free ffps_ref.ffps == the module's inds exactly, "
            "all picks distinct" % (B, N, C, NPOINT))
    print(line)


if __name__ == "__main__":
    main()

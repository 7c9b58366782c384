"""Fixture G19 — MulTransformerBlock (multitransformer.py:11-76), run against /root/reference in the build container like
make_golden.py; only arrays and key names are committed.

  blocks  (heads, layers) in tests/multitransformer_ref.BLOCKS at N = 128 and 64, one cloud whose second half repeats the
          first (duplicated points): res[..., ::4] and a sample (points ::16, channels ::8) of the last layer's attn in the reference's
          (B*heads, N, k, hd) layout; weights from fill_state_dict_ with the LayerNorm weights redrawn as 1 + 0.1 N(0,1)
  train   one training-mode forward and backward of the (4, 2) block with a seeded linear loss: every parameter's gradient
          norm, the full fc_gamma.0.weight and norm1.weight gradients of both layers, rows ::8 of the last proj.weight gradient
  tracker the reference tracker from ptt.yaml with both TRANSFORMER_BLOCKs = MulTransformerBlock (4 heads, 2 layers) on
          synth.frames inputs: the G6 output set and the state_dict key / shape list
Inputs are not stored: the tests regenerate them from the same seeds (tests/multitransformer_ref.py).

    python tests/golden/make_golden_g19.py        # writes tests/golden/G19_multitransformer.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests.golden import make_golden as MG          # noqa: E402
from tests import multitransformer_ref as M         # noqa: E402
from ptt_amd import synth                           # noqa: E402

SEED_TRAIN, SEED_TRACKER = 1990, 1919


def main():
    EasyDict = MG._install_stubs()                  # thop, pointnet2_ops, easydict
    sys.path.insert(0, MG.REF)
    from ptt.models.transformer_block.multitransformer import MulTransformerBlock as RefMTB
    torch.manual_seed(0)
    out = {}
    for heads, layers in M.BLOCKS:
        for N in M.SIZES:
            seed = M.block_seed(heads, layers, N)
            blk = M.seeded_(RefMTB(256, 512, 16, heads, layers), seed).eval()
            xyz, f = M.block_inputs(seed, 1, N)
            with torch.no_grad():
                res, attn = blk(torch.from_numpy(xyz), torch.from_numpy(f))
            tag = "h%d_l%d_n%d" % (heads, layers, N)
            out["res_" + tag] = res[..., ::4].contiguous().numpy()
            out["attn_" + tag] = attn[:, ::16, :, ::8].contiguous().numpy()
            if (heads, layers) == M.TRAIN and N == M.SIZES[0]:
                out["keys_block"] = np.array(list(blk.state_dict().keys()))
                out["shapes_block"] = np.array([str(tuple(v.shape)) for v in blk.state_dict().values()])

    # ---------------- training-mode forward + backward of the (4, 2) block ----------------
    heads, layers = M.TRAIN
    blk = M.seeded_(RefMTB(256, 512, 16, heads, layers), SEED_TRAIN).train()
    xyz, f = M.block_inputs(SEED_TRAIN, 2, 64)
    res, _ = blk(torch.from_numpy(xyz), torch.from_numpy(f))
    loss = (res * M.loss_weights(SEED_TRAIN, tuple(res.shape))).sum()
    loss.backward()
    names = [n for n, p in blk.named_parameters()]
    out.update(train_loss=np.float64(loss.item()), train_names=np.array(names),
               train_grad_norms=np.array([p.grad.double().norm().item() for p in blk.parameters()]),
               train_res=res.detach()[..., ::4].contiguous().numpy())
    for i in range(layers):
        L = blk.layers[i]
        out["train_g_fc_gamma0_w_%d" % i] = L.fc_gamma[0].weight.grad.numpy()
        out["train_g_norm1_w_%d" % i] = L.norm1.weight.grad.numpy()
    out["train_g_proj_w_last_rows8"] = blk.layers[layers - 1].proj.weight.grad[::8].contiguous().numpy()

    # ---------------- the tracker with both blocks = MulTransformerBlock(4 heads, 2 layers) ----------------
    from ptt.config import cfg_from_yaml_file as ref_cfg_from_yaml
    from ptt.models import build_network as ref_build_network
    from ptt_amd.config import StubDataset
    rcfg = ref_cfg_from_yaml(os.path.join(MG.REF, "tools/cfgs/kitti_models/ptt.yaml"), EasyDict())
    M.tracker_cfg(rcfg.MODEL)
    ref_model = M.seeded_(ref_build_network(rcfg.MODEL, 1, StubDataset()), SEED_TRACKER).eval()
    s, t = synth.frames(SEED_TRACKER, 2, 1024, 512)
    with torch.no_grad():
        o = ref_model({'search_points': torch.from_numpy(s), 'template_points': torch.from_numpy(t), 'batch_size': 2})
    keys = sorted(ref_model.state_dict().keys())
    out.update(tracker_seed=SEED_TRACKER, tracker_keys=np.array(keys),
               tracker_shapes=np.array([str(tuple(ref_model.state_dict()[k].shape)) for k in keys]),
               **{"tracker_" + k: o[k].numpy() for k in ('search_inds', 'template_inds', 'cosine_feats', 'pred_centroids_cls',
                                                         'pred_centroids_votes', 'votes_feats', 'pred_box_center',
                                                         'pred_box_data')})
    path = os.path.join(HERE, "G19_multitransformer.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(keys), "tracker state_dict keys")


if __name__ == "__main__":
    main()

"""Mirror of ptt/models/backbones_3d/pointnet2/pointnet2_modules.py: PointnetSAModuleVotes (:22-90).

Same constructor, attributes (`grouper`, `mlp_module`, `sample_method`), state_dict keys and
`forward(xyz, features, npoint, inds=None) -> (new_xyz, new_features, inds_int64)` contract.

Two execution paths, chosen per call:
  * eval mode on a HIP device (inference / tracking): sample -> ball query -> ONE fused kernel
    (ptt_sa_fused_fwd_f32: group, centre-subtract, /radius, concat, 3x[1x1 conv + folded BN +
    ReLU] on fp32 MFMA, max over nsample). The grouped (B,C,M,ns) tensors the reference
    materialises (pointnet2_utils.py:351-361) never exist. Output features are stored
    point-major (B,M,C) and returned as the (B,C,M) transposed view, which is also the layout
    the next level gathers from with coalesced loads.
  * training mode (BatchNorm needs batch statistics): the reference's op sequence on the HIP
    ops + stock torch conv/BN, with autograd through gather/group.
"""
import os
from typing import List

import torch
import torch.nn as nn
import torch.nn.functional as F

from .... import ops, train_ops
from ....param_cache import (DropsCachesOnModeChange, FoldedLayer, ParamCache, conv_bn_tensors, fold_conv_bn,
                             index_table)
from . import pointnet2_utils
from . import pytorch_utils as pt_utils

# Fewest balls (B * M) of a launch that `compact=True` sends to the compact stream kernel. The compact call is three
# launches and never takes less than 23 us; the dense kernel takes 16-18 us up to 512 balls. Measured at the search
# branch's last level (N = 256, M = 128; graph-replayed, us per call, dense / compact;
# profiles/sa2c_stream_dense_vs_compact.log):
#   balls            128 (one frame)   512           1024 (8 frames)   2048          6144 (48 frames)
#   car (1.4 hits)   16.2 / 23.1       17.5 / 23.1   31.0 / 23.4       56.0 / 23.7   155.1 / 37.7
#   ped (25 hits)    15.9 / 22.5       17.7 / 23.8   30.4 / 34.2       52.9 / 58.2   148.1 / 133.8
# Below 1024 balls dense always wins (one tracklet frame is a chain of dependent launches: +6.5 us and two more launches
# per level); at 1024 sparse balls gain 8 us and full ones lose 4; from 2048 sparse balls gain 32 us or more against 5 lost
# on full ones (scripts/sa_stream_compact_bench.py). One tracklet frame never reaches this gate: its path does not pass
# `compact` at all (docs/experiments.md has its latency against the parent).
STREAM_COMPACT_MIN_BALLS = 2048
# ... and the most points per cloud of the level (N), a proxy for ball density: the 16384-point stress clouds have 4096
# points at the last search level and 22.5 real hits per ball. Measured with this gate lifted: the stress step 23.09 / 23.11
# -> 23.75 / 23.76 ms (+2.8 %, two lines each, same session; spread 0.03 ms), although the launch alone costs the same
# (1539 dense / 1532 compact us). Every car / ped / train level has at most 512 points.
STREAM_COMPACT_MAX_POINTS = 1024
PRECISIONS = ('fp32', 'bf16x2')
# Fewest balls (B * M) of a launch that precision 'bf16x2' sends to the split-bf16 stream kernel (ptt_sa_stream_split_f32).
# The rule is the pair kernel's (transformer_block/variants.py, SPLIT_DISPATCH): the split kernel is dispatched only where
# scripts/sa_split_timing.py shows it faster than sa_stream_kernel<32> by more than the fp32 arm's own spread; a launch below
# this count runs in fp32 with a note. Measured (kernel launch alone, us, fp32 / split; fp32 arm's min - max spread in brackets):
#   balls   256 (one frame, 512 -> 256)   3072 (48 x 64)     6144 (48 x 128)     12288 (48 x 256)    131072 (stress)
#           19.7 / 12.6 [0.4]             84.4 / 35.0 [6.4]  160.2 / 60.7 [16]   312.9 / 113.3 [39]  3079 / 1217 [21]
# The split kernel wins at every count by many spreads, so the threshold is 0: every dense stream launch is dispatched
# (DESIGN.md "Split-bf16 stream kernel", profiles/sa_split_timing.json).
SPLIT_STREAM_MIN_BALLS = 0


class PointnetSAModuleVotes(DropsCachesOnModeChange, nn.Module):
    def __init__(self, *, mlp: List[int], radius: float = None, nsample: int = None, bn: bool = True,
                 use_xyz: bool = True, normalize_xyz: bool = False, sample_uniformly: bool = False,
                 sample_method='fps'):
        super().__init__()
        self.radius = radius
        self.nsample = nsample
        self.mlp_module = None
        self.use_xyz = use_xyz
        self.normalize_xyz = normalize_xyz
        self.sample_uniformly = sample_uniformly
        self.grouper = pointnet2_utils.QueryAndGroup(radius, nsample, use_xyz=use_xyz, ret_grouped_xyz=True,
                                                     normalize_xyz=normalize_xyz, sample_uniformly=sample_uniformly,
                                                     ret_unique_cnt=False)
        mlp_spec = mlp
        if use_xyz and len(mlp_spec) > 0:
            mlp_spec[0] += 3        # in place on the caller's list, exactly as the reference does (:51-53)
        self.mlp_module = pt_utils.SharedMLP(mlp_spec, bn=bn)
        self.sample_method = sample_method
        self._fused_cache = ParamCache()
        self._split_cache = ParamCache()   # the split-bf16 packs of layers 1 and 2: built only under precision 'bf16x2'
        self._precision = 'fp32'
        self.centres_knn_k = 0      # > 0: a caller that runs a TransformerBlock on this level's centres (the box head) wants their
        self.centres_knn = None     #      kNN; at one frame it is formed in the sampling launch and left here (knn_idx, rel)

    # ------------------------------------------------------------------ arithmetic of the dense stream level
    @property
    def precision(self):
        """'fp32' (default) or 'bf16x2': an eval-mode call that would reach the dense streamed kernel (hoisted 128-channel layer 0,
        128 -> 128 -> 256, 32 neighbours) takes the operands of its two GEMMs as two bf16 pieces each (ptt_sa_stream_split_f32).
        Every other call — SA0, a compact-gated level, the one-frame forms, other widths, training — stays fp32 either way."""
        return getattr(self, '_precision', 'fp32')

    @precision.setter
    def precision(self, value):
        if value not in PRECISIONS:
            raise ValueError("PointnetSAModuleVotes.precision must be one of %s, got %r" % (", ".join(map(repr, PRECISIONS)), value))
        if value != self.precision:
            self._fused_cache.drop()    # a captured graph addressed the old mode's buffers
            self._split_cache.drop()    # the split packs exist only under 'bf16x2'
        self._precision = value

    def _name(self):
        return 'PointnetSAModuleVotes(nsample=%s, mlp=%s)' % (self.nsample, [u.conv.weight.shape[0] for u in self.mlp_module
                                                                           if hasattr(u, 'conv')])

    def _split_params(self, device):
        """-> dict(w1s, shift1, w2s, shift2, relu2): layers 1 and 2 of the SharedMLP for ops.sa_stream_split — the BatchNorm scale
        folded into the weights in float32 (the values the fp32 pack holds), then ops.pack_weight_split."""
        return self._split_cache.get(conv_bn_tensors(self.mlp_module), device, self._fold_split)

    def _fold_split(self):
        packs = []
        for unit in (self.mlp_module[1], self.mlp_module[2]):
            scale, shift = fold_conv_bn(unit)
            w = unit.conv.weight
            wq = w if scale is None else w * scale.view(-1, 1, 1, 1)
            packs.append((ops.pack_weight_split(wq), shift))
        return dict(w1s=packs[0][0], shift1=packs[0][1], w2s=packs[1][0], shift2=packs[1][1],
                    relu2=hasattr(self.mlp_module[2], 'activation'))

    def _split_reason(self, features, hoist, layers, B, M, compact_gated):
        """None when this eval-mode call runs the split-bf16 stream kernel, else why it stays on the fp32 kernels."""
        if features is None:
            return 'no point features (SA0): sa_lds_kernel is fp32 only'
        if (hoist is None or hoist[2] != 128 or self.nsample != 32 or len(layers) != 3
                or (layers[1].cin, layers[1].cout, layers[2].cin, layers[2].cout) != (128, 128, 128, 256) or not layers[1].relu
                or layers[1].scale is not None or layers[2].scale is not None):
            return 'other widths than a hoisted 128-channel layer 0, 128 -> 128 -> 256 and 32 neighbours: fp32 only'
        if compact_gated:
            return 'compact-gated level: sa_stream_compact_kernel is fp32 only'
        if B * M < SPLIT_STREAM_MIN_BALLS:
            return 'fewer than %d balls: the split-bf16 stream kernel is not faster there, not dispatched' % SPLIT_STREAM_MIN_BALLS
        return None

    # ------------------------------------------------------------------ sampling (reference :63-77)
    def _sample(self, xyz, features, npoint):
        if self.sample_method == 'fps':
            return pointnet2_utils.furthest_point_sample(xyz, npoint)
        if self.sample_method in ('rs', 'sequence'):
            return index_table(xyz.size(0), npoint, xyz.device, torch.int32)
        if self.sample_method == 'ffps':
            # furthest points in [xyz ; features] space (reference :64-67, a branch its extension could never run: it has no
            # furthest_point_sampling_with_dist) — matrix-free, the features read in place whatever their layout
            if features is None:
                raise ValueError("sample_method 'ffps': a level without point features cannot sample in feature space "
                                 "(use 'fps' for it)")
            return ops.feature_fps(xyz.contiguous(), features.detach(), npoint)
        raise NotImplementedError(self.sample_method)

    # ------------------------------------------------------------------ fused-path parameters
    def _fusable(self, xyz, features):
        """Eval mode on a HIP device, a shape ptt_sa_fused_fwd_f32 instantiates, and no autograd graph being recorded
        (the kernels have none: with gradients enabled and anything requiring them the call stays on the
        differentiable stock-torch path, as the reference's eval mode is). An eval-mode HIP call that is turned away
        says so once (ops.note_unfused)."""
        if self.training or not xyz.is_cuda:
            return False
        name = self._name()
        if ops.autograd_recording(self, xyz, features):
            return ops.note_unfused(name, 'autograd is recording (wrap inference in torch.no_grad())')
        if self.sample_uniformly or self.nsample not in (16, 32, 64):
            return ops.note_unfused(name, 'nsample must be 16, 32 or 64 and sample_uniformly off')
        if xyz.dtype != torch.float32 or (features is not None and features.dtype != torch.float32):
            return ops.note_unfused(name, 'inputs must be float32')
        if len(self.mlp_module) > 4:
            return ops.note_unfused(name, 'more than 4 SharedMLP layers')
        for unit in self.mlp_module:
            conv = getattr(unit, 'conv', None)
            if conv is None or conv.kernel_size != (1, 1) or conv.weight.shape[0] % 32 != 0 or conv.weight.shape[0] > 256:
                return ops.note_unfused(name, 'layer widths must be multiples of 32, at most 256, 1x1 convolutions')
            if list(unit._modules.keys())[0] != 'conv':     # pre-activation units are not folded
                return ops.note_unfused(name, 'pre-activation units')
        return True

    def _fused_params(self, device):
        """-> ([FoldedLayer, ...], hoist): the SharedMLP folded for ops.sa_fused_forward, and layer 0 split for the hoisted form
        (wf_packed, wx, c0, relu0) or None."""
        return self._fused_cache.get(conv_bn_tensors(self.mlp_module), device, self._fold)

    def _fold(self):
        layers, scale0 = [], None
        for li, unit in enumerate(self.mlp_module):
            w = unit.conv.weight
            cout, cin = w.shape[0], w.shape[1]
            rot = 3 if (li == 0 and self.use_xyz and cin > 3) else 0     # kernel row layout is [features | xyz]
            scale, shift = fold_conv_bn(unit)
            scale0 = scale if li == 0 else scale0                        # the hoisted layer 0 folds it into its own two packs
            # the BatchNorm scale is folded into the packed weights: the kernels then start their accumulators at
            # `shift` and the epilogue is a bare ReLU (every vector-ALU instruction outside the MFMA loop costs
            # matrix time on gfx950)
            wq = w if scale is None else w * scale.view(-1, 1, 1, 1)
            layers.append(FoldedLayer(ops.pack_weight(wq, rot), None, shift, cin, cout, hasattr(unit, 'activation')))
        # Layer 0 is linear in [rel ; f_n]: its feature half is evaluated once per POINT (N rows on the linear
        # kernel) instead of once per (centre, neighbour) row; the kernel adds the 3 relative-coordinate terms.
        hoist = None
        w0 = self.mlp_module[0].conv.weight
        if (self.use_xyz and len(layers) >= 2 and w0.shape[1] > 3 and layers[0].cout <= 256
                and os.environ.get('PTT_SA_HOIST', '1') != '0'):
            w2 = w0.reshape(w0.shape[0], w0.shape[1]).float()
            wx = w2[:, 0:3] if scale0 is None else w2[:, 0:3] * scale0[:, None]
            # the BatchNorm scale folded into both halves of layer 0 (no per-value scale in the linear launch's epilogue)
            wf = w2[:, 3:] if scale0 is None else w2[:, 3:] * scale0[:, None]
            hoist = (ops.pack_weight(wf.contiguous()), wx.t().contiguous(), layers[0].cout, layers[0].relu)
        return layers, hoist

    # ------------------------------------------------------------------ forward (reference :57-90)
    def forward(self, xyz: torch.Tensor, features: torch.Tensor, npoint: int, inds: torch.Tensor = None, pre=None,
                compact: bool = False):
        """`pre` (an extension of the reference signature, eval mode on a HIP device only): (new_xyz, idx, inds64) of this level
        already computed by the caller — the backbone forms the ball queries of all three levels of a branch in one launch
        when it runs one tracklet frame (ops.sa_levels_point_jobs).
        `compact` (same conditions): a level WITH point features pools each ball's real hits only (the stream shape of
        ops.sa_fused_forward, bitwise the same output) when the launch has at least STREAM_COMPACT_MIN_BALLS balls."""
        self.centres_knn = None
        if self._fusable(xyz, features):
            return self._forward_fused(xyz, features, npoint, inds, pre, compact)
        if self.precision == 'bf16x2' and xyz.is_cuda:
            ops.note_precision_fallback(self._name(), 'training (and every call the fused eval path turns away) runs in fp32')
        return self._forward_train(xyz, features, npoint, inds)

    def _forward_fused(self, xyz, features, npoint, inds, pre, compact):
        """Eval mode on a HIP device: sampling and ball query (unless `pre` brings them), then the SharedMLP and the max over
        the neighbours in ops.sa_fused_forward — or, for a handful of frames with a hoisted layer 0, in two row-job launches."""
        if (pre is None and inds is None and self.sample_method == 'fps' and xyz.shape[1] <= 256 and npoint <= 128
                and xyz.shape[0] * npoint * self.nsample <= ops.ONE_FRAME_MAX_SA_ROWS and self.centres_knn_k <= npoint):
            # a handful of frames (vote_aggregation at one tracklet frame): sampling, centre selection, ball query and the
            # centres' kNN in ONE launch (ptt_fps_ball_knn_f32) instead of three
            xyz = xyz.contiguous()
            inds, inds64, new_xyz, idx, self.centres_knn = ops.fps_ball_knn(xyz, npoint, self.radius, self.nsample, self.centres_knn_k)
            pre = (new_xyz, idx, inds64)
        prefix = inds is None and self.sample_method in ('rs', 'sequence')   # centres = the first npoint points
        if pre is not None:
            pass
        elif prefix:
            # 'sequence' indices are constants of (B, npoint): build them once, not four tiny kernels per call
            inds64 = index_table(xyz.size(0), npoint, xyz.device, torch.int64)
        elif inds is None:
            inds = self._sample(xyz, features, npoint)
        else:
            assert inds.shape[1] == npoint
            inds = inds.to(torch.int32)

        xyz = xyz.contiguous()
        if pre is not None:
            new_xyz, idx, inds64 = pre
        elif prefix:                                 # centres + ball query in one launch
            new_xyz, _, idx = ops.centres_ball_query(xyz, None, npoint, self.radius, self.nsample)
        else:
            new_xyz, inds64, idx = ops.centres_ball_query(xyz, inds.contiguous(), npoint, self.radius, self.nsample)
        layers, hoist = self._fused_params(xyz.device)
        split = self.precision == 'bf16x2'
        if split and (hoist is None or features is None):
            ops.note_precision_fallback(self._name(), self._split_reason(features, hoist, layers, xyz.shape[0], npoint, False))
        if hoist is not None and features is not None:
            wf_packed, wx, c0, relu0 = hoist
            rows = features.transpose(1, 2)                       # (B,N,C): contiguous when point-major
            # rows with a padded stride (the one-frame head hands over 260-float rows) are read in place
            uniform = rows.stride(2) == 1 and rows.stride(0) == rows.shape[1] * rows.stride(1)
            term = ops.linear(rows if uniform else rows.contiguous(), wf_packed, c0, None, layers[0].shift, relu=False)
            B, M, ns = xyz.shape[0], npoint, self.nsample
            if (B * M * ns <= ops.ONE_FRAME_MAX_SA_ROWS and ns in (16, 32) and len(layers) == 3 and c0 % 4 == 0 and c0 >= 192):
                # a handful of frames (vote_aggregation at one tracklet frame: 64 centres x 16 neighbours): the fused SA
                # kernel would be 16 workgroups with two chained 256 x 256 layers each (41 us); as two row-job launches
                # the 1024 grouped rows spread over the chip: layer 1 on rows built while its A tile is staged (term[idx]
                # + Wx . rel, ReLU), then layer 2 with the max over the neighbours as its epilogue
                if split:
                    ops.note_precision_fallback(self._name(), 'a handful of frames: the one-frame row-job forms are fp32 only')
                L1, L2 = layers[1], layers[2]
                h = torch.empty((B * M * ns, L1.cout), dtype=torch.float32, device=xyz.device)
                ops.row_jobs([pt_utils.layer_job(L1, prologue=3, x=term, idx=idx, xyz=xyz, centres=new_xyz, wx=wx,
                                                 radius=self.radius, ns=ns, M=M, N=xyz.shape[1], normalize_xyz=self.normalize_xyz,
                                                 pro_relu=relu0, out=h)])
                pooled = torch.empty((B, M, L2.cout), dtype=torch.float32, device=xyz.device)
                ops.row_jobs([pt_utils.layer_job(L2, x=h, epilogue=2, ns=ns, M=M, out=pooled)])
                return new_xyz, pooled.transpose(1, 2), inds64
            compact_gated = bool(compact) and B * M >= STREAM_COMPACT_MIN_BALLS and xyz.shape[1] <= STREAM_COMPACT_MAX_POINTS
            if split:
                reason = self._split_reason(features, hoist, layers, B, M, compact_gated)
                if reason is None:
                    S = self._split_params(xyz.device)
                    new_features = ops.sa_stream_split(xyz, new_xyz, idx, (term, wx, relu0), S['w1s'], S['shift1'], S['w2s'],
                                                       S['shift2'], self.radius, self.normalize_xyz, relu2=S['relu2'])
                    return new_xyz, new_features, inds64
                ops.note_precision_fallback(self._name(), reason)
            new_features = ops.sa_fused_forward(xyz, new_xyz, idx, None, layers[1:], self.radius, True,
                                                self.normalize_xyz, point_major_out=True, l0=(term, wx, relu0),
                                                compact=compact_gated)
        else:
            # the level without point features (SA0) pools each ball's distinct rows only: same bits, a fraction of
            # the rows (ball-query padding and the resampled clouds' repeated points)
            new_features = ops.sa_fused_forward(xyz, new_xyz, idx, features, layers, self.radius,
                                                self.use_xyz, self.normalize_xyz, point_major_out=True,
                                                compact=features is None)
        return new_xyz, new_features, inds64

    def _forward_train(self, xyz, features, npoint, inds):
        """Training mode, the CPU, and the eval-mode calls _fusable turned away: the hoisted training forms of
        train_ops where they apply, else the reference's op sequence."""
        if inds is None:
            inds = self._sample(xyz, features, npoint)
        else:
            assert inds.shape[1] == npoint
            inds = inds.to(torch.int32)
        hoist = (self.use_xyz and not self.sample_uniformly and self.nsample * npoint <= 16384
                 and train_ops.usable(self.mlp_module, xyz if features is None else features)
                 and self.mlp_module[0].conv.weight.shape[0] % 4 == 0)
        if hoist and not xyz.requires_grad and inds.dtype == torch.int32:
            # training mode on a HIP device, fixed coordinates (the backbone): centres + ball query in one launch, then
            # layer 0 per (centre, neighbour) row in one more (train_ops.sa_level_hoisted -> ptt_sa_z0_rows_f32) — also for
            # the level without point features, whose first convolution is the three coordinate channels alone
            new_xyz, inds64, idx = ops.centres_ball_query(xyz.contiguous(), inds.contiguous(), npoint, self.radius, self.nsample)
            y = train_ops.sa_level_hoisted(xyz, new_xyz, features, idx, self.mlp_module, self.radius, self.normalize_xyz)
            return new_xyz, y, inds64
        xyz_flipped = xyz.transpose(1, 2).contiguous()
        new_xyz = pointnet2_utils.gather_operation(xyz_flipped, inds).transpose(1, 2).contiguous()
        if hoist and features is not None:
            # learnable coordinates (the box head's vote aggregation): layer 0 hoisted to one row per POINT, gradients to
            # the coordinates through the grouping / gather operators
            idx = pointnet2_utils.ball_query(self.radius, self.nsample, xyz, new_xyz)
            y = train_ops.sa_level_hoisted(xyz, new_xyz, features, idx, self.mlp_module, self.radius, self.normalize_xyz)
            return new_xyz, y, inds.to(torch.int64)
        grouped_features, grouped_xyz = self.grouper(xyz, new_xyz, features)      # (B,C,M,ns)
        if train_ops.usable(self.mlp_module, grouped_features):
            # training mode on a HIP device: SharedMLP (batch-statistics BatchNorm) + the max over the neighbours, forward
            # and backward, on the hand-written row kernels (ptt_amd/train_ops.py)
            return new_xyz, train_ops.shared_mlp_pool(grouped_features, self.mlp_module, pool_dim=3), inds.to(torch.int64)
        y = self.mlp_module(grouped_features)
        # reference: F.max_pool2d(y, kernel_size=[1, nsample]).squeeze(-1) (:85-88); max over the last axis routes the
        # gradient to one arg-max the same way and avoids torch's NCHW pooling kernel (6 ms per training step here)
        y = y.max(dim=3)[0]                                                       # (B,Cout,M)
        return new_xyz, y, inds.to(torch.int64)

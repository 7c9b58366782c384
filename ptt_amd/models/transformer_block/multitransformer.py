"""Mirror of ptt/models/transformer_block/multitransformer.py: MulHeadTransformerLayer (:11-63) and MulTransformerBlock
(:66-76), the second choice the shipped config names for both transformer blocks (`NAME: MulTransformerBlock`, with
N_HEADS and N_LAYERS).

One layer is TransformerBlock's vector attention split into `heads` heads of hd = d_model / heads channels:
    attn_ij = softmax_j( fc_gamma(q_i - k_j + delta_ij per head) / sqrt(hd) )      fc_gamma: ONE hd x hd MLP all heads share
    res_i   = LayerNorm_dpoints( fc2( LayerNorm_D( proj( concat_h sum_j attn_ij * (v_j + delta_ij) ) ) ) ) + features_i
and the block runs `layers` deep copies in sequence. Parameter names (layers.{i}.fc1, fc2, fc_delta.{0,2}, fc_gamma.{0,2},
w_qs, w_ks, w_vs, proj, norm1, norm2) are the reference's, so its checkpoints load unchanged.

Eval mode on a HIP device (float32; d_model 128 / 256 with k 8 / 16 / 32, d_model 512 with k 16; heads 1 / 2 / 4 / 8 with
hd >= 32, i.e. not 8 heads at d_model 128; a number of points >= k that is a multiple of 32 // k) runs one kNN per block
and per layer: the q|k|v projection with fc1 folded in, the attention (the pair kernel's per-head form, whose
fc_gamma GEMMs read only their head's hd input channels; at (512, 16) one frame without attn takes the row-job chain of
TransformerBlock with fc_gamma expanded to its block-diagonal D x D form — that chain has 512 channels and 16 neighbours built
in, every other shape runs the pair kernel whatever B * N is), proj, a LayerNorm, fc2 and a LayerNorm with the residual. Return contract as
TransformerBlock: `forward(xyz, features, knn=None, want_attn=True) -> (res, attn)`, attn the LAST layer's
(B*heads, N, k, hd) tensor, or None when the caller opts out with want_attn=False.

Training mode on a HIP device (train_ops.mul_block_usable: float32, the same (d_model, k, heads) envelope, no dropout) runs on the
row kernels of ptt_amd/train_ops.py as TransformerBlock's training step does: one kNN and one CSR order of its indices per block,
per layer the Linears on the row GEMMs, the attention core with the heads' shared fc_gamma, and both LayerNorms on the training
LayerNorm kernels. Everything else (CPU, other shapes, a non-zero dropout) follows the reference's ops in stock torch."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops, train_ops
from ...param_cache import ParamCache
from ..model_utils import get_clones, index_points, square_distance
from .variants import PER_LAYER_MAX_POINTS, SPATIAL_ORDER_MIN_POINTS, _rows2d

FUSED_HEADS = (1, 2, 4, 8)          # the head counts ptt_pt_attn_pair_f32 instantiates, where hd = d_model / heads >= 32
ROW_JOB_CHAIN = (512, 16)           # (d_model, k) of the one-frame row-job chain (rowjobs.hip: both are built in)


class MulHeadTransformerLayer(nn.Module):
    def __init__(self, d_points, d_model, k, heads, drop=0.) -> None:
        super().__init__()
        self.heads = heads
        head_dim = d_model // heads
        self.fc1 = nn.Linear(d_points, d_model)
        self.fc2 = nn.Linear(d_model, d_points)
        self.fc_delta = nn.Sequential(nn.Linear(3, d_model), nn.ReLU(), nn.Linear(d_model, d_model))
        self.fc_gamma = nn.Sequential(nn.Linear(head_dim, head_dim), nn.ReLU(), nn.Linear(head_dim, head_dim))
        self.w_qs = nn.Linear(d_model, d_model, bias=False)
        self.w_ks = nn.Linear(d_model, d_model, bias=False)
        self.w_vs = nn.Linear(d_model, d_model, bias=False)
        self.proj = nn.Linear(d_model, d_model, bias=False)
        self.proj_drop = nn.Dropout(drop)
        self.k = k
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_points)
        self.d_model = d_model
        self.d_points = d_points
        self.head_dim = head_dim
        self._cache = ParamCache()

    # ---------------------------------------------------------------- fused-path parameters
    def _params(self):
        ts = [self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias, self.w_qs.weight, self.w_ks.weight,
              self.w_vs.weight, self.fc_delta[0].weight, self.fc_delta[0].bias, self.fc_delta[2].weight,
              self.fc_delta[2].bias, self.fc_gamma[0].weight, self.fc_gamma[0].bias, self.fc_gamma[2].weight,
              self.fc_gamma[2].bias, self.proj.weight, self.norm1.weight, self.norm1.bias, self.norm2.weight, self.norm2.bias]
        return self._cache.get(ts, ts[0].device, self._pack)

    def _pack(self):
        f = lambda t: t.detach().float().contiguous()
        H = self.heads
        # fc1 folded into the q|k|v projection, as TransformerBlock._params does (product in f64)
        wqkv = torch.cat([self.w_qs.weight, self.w_ks.weight, self.w_vs.weight], 0).double()
        # the one-frame chain runs fc_gamma on the row-job kernel as its block-diagonal D x D expansion (diagonal blocks =
        # the shared hd x hd weight); the pair kernel reads the hd x hd weights themselves
        blockdiag = lambda wt: torch.block_diag(*([f(wt)] * H)).contiguous()
        chain = {}
        if (self.d_model, self.k) == ROW_JOB_CHAIN:
            chain = dict(wg1_bd=ops.pack_weight(blockdiag(self.fc_gamma[0].weight)),
                         wg2_bd=ops.pack_weight(blockdiag(self.fc_gamma[2].weight)))
        return dict(
            qkv=ops.pack_weight((wqkv @ self.fc1.weight.double()).float().contiguous()),
            qkv_b=(wqkv @ self.fc1.bias.double()).float().contiguous(),
            wd1=ops.pack_delta0(self.fc_delta[0].weight, self.fc_delta[0].bias),
            wd2=ops.pack_weight(self.fc_delta[2].weight), bd2=f(self.fc_delta[2].bias),
            wg1=ops.pack_weight(self.fc_gamma[0].weight), wg2=ops.pack_weight(self.fc_gamma[2].weight),
            bg1=f(self.fc_gamma[0].bias).repeat(H).contiguous(), bg2=f(self.fc_gamma[2].bias).repeat(H).contiguous(),
            w1b=torch.cat((f(self.fc_delta[0].weight), f(self.fc_delta[0].bias)[:, None]), 1).contiguous(),
            proj=ops.pack_weight(self.proj.weight),
            fc2=ops.pack_weight(self.fc2.weight), fc2_b=f(self.fc2.bias),
            n1w=f(self.norm1.weight), n1b=f(self.norm1.bias), n2w=f(self.norm2.weight), n2b=f(self.norm2.bias), **chain)

    def _fused(self, xyz, features, knn_idx, rel, want_attn, order):
        """One layer on the HIP kernels; the caller has checked MulTransformerBlock._fusable and formed the kNN."""
        P = self._params()
        D, H, k = self.d_model, self.heads, self.k
        B, N = xyz.shape[0], xyz.shape[1]
        dev = xyz.device
        if (D, k) == ROW_JOB_CHAIN and B * N <= PER_LAYER_MAX_POINTS and not want_attn:
            # one frame: TransformerBlock's row-job chain (variants.py: the per-layer form), fc_gamma block-diagonal
            qkv = torch.empty((B, N, 3 * D), dtype=torch.float32, device=dev)
            pos = torch.empty((B * N * k, D), dtype=torch.float32, device=dev)
            g = torch.empty_like(pos)
            res = torch.empty((B, N, D), dtype=torch.float32, device=dev)
            knn2 = knn_idx.view(-1, k)
            ops.row_jobs([ops.row_job(P['wd2'], D, prologue=1, rel=rel.view(-1, 3), w1=P['w1b'], K=D, shift=P['bd2'], out=pos),
                          ops.row_job(P['qkv'], 3 * D, x=features, shift=P['qkv_b'], out=qkv)])
            ops.row_jobs([ops.row_job(P['wg1_bd'], D, prologue=2, qkv=qkv, knn=knn2, pos=pos, q_off=0, k_off=D, N=N, K=D,
                                      shift=P['bg1'], act=1, out=g)])
            ops.row_jobs([ops.row_job(P['wg2_bd'], D, x=g, epilogue=1, qkv=qkv, knn=knn2, pos=pos, v_off=2 * D, N=N,
                                      sm_scale=1.0 / np.sqrt(self.head_dim), out=res)])
            attn = None
        else:
            qkv = ops.linear(features, P['qkv'], 3 * D, None, P['qkv_b'])
            res, attn = ops.pt_attn_pair(xyz, knn_idx, qkv, P['wd1'], P['wd2'], P['bd2'], P['wg1'], P['bg1'], P['wg2'],
                                         P['bg2'], D, want_attn, rel=rel, order=order, heads=H)
        # res = norm1(proj(res)); out = norm2(fc2(res)) + features   (multitransformer.py:59-60; dropout 0)
        r = ops.linear(res, P['proj'], D)
        ops.layernorm(r, P['n1w'], P['n1b'], self.norm1.eps, out=r)
        o = ops.linear(r, P['fc2'], self.d_points, None, P['fc2_b'])
        ops.layernorm(o, P['n2w'], P['n2b'], self.norm2.eps, residual=features, out=o)
        return o, attn

    def _train_rows(self, features, knn_idx, rel, order, start, want_attn):
        """One layer's training step on the row kernels (train_ops); the caller has checked train_ops.mul_block_usable and formed
        the kNN, the relative coordinates and the CSR order of the neighbour indices (shared by every layer of the block)."""
        H = self.heads
        x = train_ops.rows_linear(self.fc1, features)
        q, kf, vf = (train_ops.rows_linear(m, x) for m in (self.w_qs, self.w_ks, self.w_vs))
        pos_enc = train_ops.rows_mlp2(self.fc_delta, rel)                          # (B,N,k,D)
        res, attn = train_ops.attn_core(self.fc_gamma, q, kf, vf, knn_idx, pos_enc, 1.0 / np.sqrt(self.head_dim), order, start, heads=H)
        res = train_ops.rows_layernorm(self.norm1, train_ops.rows_linear(self.proj, res))
        res = train_ops.rows_layernorm(self.norm2, train_ops.rows_linear(self.fc2, res), residual=features)
        if not want_attn:
            return res, None
        B, N, k, D = attn.shape                                                    # head-major channels -> (B*heads, N, k, hd)
        return res, attn.view(B, N, k, H, D // H).permute(0, 3, 1, 2, 4).flatten(0, 1)

    def forward(self, xyz, features):
        """The reference's op sequence in stock torch (multitransformer.py:37-63): CPU, training and the calls outside the
        fused envelope. `_rows2d` and the neighbour-axis sum instead of einsum, as TransformerBlock does."""
        dists = square_distance(xyz, xyz)
        knn_idx = dists.argsort()[:, :, :self.k]
        knn_xyz = index_points(xyz, knn_idx)
        pre = features
        x = self.fc1(features)
        B, N, C = x.shape
        H = self.heads
        query, key, value = self.w_qs(x), index_points(self.w_ks(x), knn_idx), index_points(self.w_vs(x), knn_idx)
        query = query.view(B, N, H, -1).permute(0, 2, 1, 3).flatten(0, 1)
        pos_enc = _rows2d(self.fc_delta, xyz[:, :, None] - knn_xyz)
        pos_enc, key, value = (t.view(B, N, t.shape[2], H, -1).permute(0, 3, 1, 2, 4).flatten(0, 1)
                               for t in (pos_enc, key, value))
        attn = _rows2d(self.fc_gamma, query[:, :, None] - key + pos_enc)
        attn = F.softmax(attn / np.sqrt(key.size(-1)), dim=-2)
        res = (attn * (value + pos_enc)).sum(dim=2)                        # einsum('bmnf,bmnf->bmf'), :56
        if H > 1:
            res = res.permute(0, 2, 1).reshape(B, C, N).permute(0, 2, 1)
        res = self.norm1(self.proj_drop(self.proj(res)))
        res = self.norm2(self.fc2(res)) + pre
        return res, attn


class MulTransformerBlock(nn.Module):
    def __init__(self, d_points, d_model, k, heads, layers, **kwargs):
        super().__init__()
        transformer_layer = MulHeadTransformerLayer(d_points, d_model, k, heads)
        self.layers = get_clones(transformer_layer, layers)
        self.k = k
        self.heads = heads
        self.d_model = d_model
        self.d_points = d_points

    def _fusable(self, xyz, features):
        """As TransformerBlock._fusable, with the (d_model, k, heads) envelope of the multi-head pair kernel (ops.mul_block_supported)."""
        if self.training or not xyz.is_cuda:
            return False
        name = 'MulTransformerBlock(d_model=%d, k=%d, heads=%d)' % (self.d_model, self.k, self.heads)
        if ops.autograd_recording(self, xyz, features):
            return ops.note_unfused(name, 'autograd is recording (wrap inference in torch.no_grad())')
        if self.heads not in FUSED_HEADS:
            return ops.note_unfused(name, 'ptt_pt_attn_pair_f32 instantiates heads %s' % (FUSED_HEADS,))
        if not ops.mul_block_supported(self.d_model, self.k, self.heads):
            return ops.note_unfused(name, 'MulTransformerBlock runs fused at d_model 128, 256 x k 8, 16, 32 and d_model 512 x k 16, '
                                          'with d_model / heads >= 32')
        if xyz.shape[1] % (32 // self.k) != 0 or xyz.shape[1] < self.k:
            return ops.note_unfused(name, 'needs a number of points >= k that is a multiple of %d (got %d)'
                                    % (32 // self.k, xyz.shape[1]))
        if features.dtype != torch.float32 or xyz.dtype != torch.float32:
            return ops.note_unfused(name, 'inputs must be float32')
        return True

    def forward(self, xyz, features, knn=None, want_attn=True):
        """-> (last layer's output (B,N,d_points), last layer's attn (B*heads,N,k,hd) or None), as the reference
        (multitransformer.py:72-76). `knn` and `want_attn` as TransformerBlock.forward; every layer reads the same kNN of
        `xyz` (the reference recomputes it per layer), and only the last layer's attention is ever written."""
        if self._fusable(xyz, features):
            xyz = xyz.contiguous()
            if knn is not None and knn[0].shape == (xyz.shape[0], xyz.shape[1], self.k):
                knn_idx, rel = knn
            else:
                knn_idx, rel = ops.knn(xyz, self.k, want_rel=True)
            big = xyz.shape[0] * xyz.shape[1] > PER_LAYER_MAX_POINTS
            order = ops.spatial_order(xyz) if big and SPATIAL_ORDER_MIN_POINTS <= xyz.shape[1] <= 8192 else None
            output, attn = features.contiguous(), None
            for i, layer in enumerate(self.layers):
                output, attn = layer._fused(xyz, output, knn_idx, rel, want_attn and i == len(self.layers) - 1, order)
            return output, attn
        if train_ops.mul_block_usable(self, xyz, features):
            # training mode on a HIP device: the row kernels of ptt_amd/train_ops.py, as TransformerBlock's training branch. kNN: the
            # HIP kernel (ascending (distance, index), a stable refinement of the reference's argsort), once for all layers
            knn_idx, rel = ops.knn(xyz.contiguous(), self.k, want_rel=True)
            if xyz.requires_grad:                                                     # the box head's proposals carry grad
                rel = train_ops._KnnRel.apply(xyz, knn_idx, rel)
            order, start = ops.scatter_csr(knn_idx.view(knn_idx.shape[0], -1), knn_idx.shape[1])
            output, attn = features, None
            for i, layer in enumerate(self.layers):
                output, attn = layer._train_rows(output, knn_idx, rel, order, start, want_attn and i == len(self.layers) - 1)
            return output, attn
        output = features
        for layer in self.layers:
            output, attn = layer(xyz, output)
        return output, attn

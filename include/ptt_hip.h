/*
 * ptt_hip.h — C ABI of libptt_hip.so, the MI355X (gfx950) implementation of PTT's
 * per-frame point-feature hot path.
 *
 * Every entry point replaces one call the reference makes into the third-party CUDA
 * extension `pointnet2_ops._ext` (reference: ptt/models/backbones_3d/pointnet2/
 * pointnet2_utils.py:24) or one pure-PyTorch module forward on the hot path; the
 * reference call site each one stands in for is cited beside it.
 *
 * Conventions
 *   - plain C: raw DEVICE pointers, sizes, a hipStream_t passed as void*.
 *   - every function returns 0 (PTT_OK) or a negative PTT_E* code; nothing throws,
 *     nothing allocates, nothing synchronises the host. Kernels are enqueued on
 *     `stream` and the call returns immediately.
 *   - caller owns all buffers (outputs and workspaces); layouts are row-major and
 *     contiguous unless a stride argument says otherwise.
 *   - thread-safe and re-entrant: no global state beyond a thread-local last-error
 *     string.
 *   - clouds are (B, N, 3) fp32 "xyz"; indices are int32 as in the reference
 *     (pointnet2_utils.py:58-85, 265-294).
 *
 * This file is also what Python binds from: ptt_amd/_lib.py reads it at import and takes the list of
 * entry points, every restype / argtypes and the integer PTT_* constants from the text below — there is
 * no second table to edit. Keep it plain C that a small parser reads: one prototype per `;`, `(void)`
 * for no parameters, scalar parameters of the types int, int32_t, uint32_t, int64_t, long long, size_t,
 * float, double and ptt_stream_t, any pointer otherwise (a new scalar type is added to CTYPES in
 * _lib.py, or the import raises); constants as `#define PTT_NAME <decimal>`. Structures are still mirrored by
 * hand in _lib.py, and tests compare those mirrors with what the C compiler makes of this file.
 */
#ifndef PTT_HIP_H
#define PTT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTT_ABI_VERSION 39

enum {
    PTT_OK = 0,
    PTT_EINVAL = -1,        /* bad size / null pointer / inconsistent descriptor   */
    PTT_EUNSUPPORTED = -2,  /* shape outside what the kernels are instantiated for */
    PTT_ELAUNCH = -3,       /* hipLaunch / runtime error, see ptt_last_error_string */
    PTT_EWORKSPACE = -4     /* workspace too small                                  */
};

typedef void* ptt_stream_t; /* hipStream_t */

int ptt_version(void);
const char* ptt_error_name(int code);
const char* ptt_last_error_string(void);

/* ---------------------------------------------------------------------------------
 * F1  furthest point sampling
 * replaces _ext.furthest_point_sampling(xyz, npoint)        pointnet2_utils.py:78
 *   xyz  (B,N,3) f32   ->  idx_out (B,npoint) i32
 * idx[0]=0; running min-dist starts at 1e10; points with x*x+y*y+z*z <= 1e-3 are
 * neither updated nor selectable; d=(dx*dx+dy*dy)+dz*dz in fp32 without FMA
 * contraction; arg-max ties -> lowest index; no candidate -> 0.
 * ------------------------------------------------------------------------------- */
int ptt_fps_f32(const float* xyz, int B, int N, int npoint, int32_t* idx_out,
                ptt_stream_t stream);
/* The same call for clouds of any size (the reference's op has no limit; ptt_fps_f32 answers PTT_EUNSUPPORTED for
 * N > 16384 or npoint > 15360): the running min-distance in `workspace` (>= B*N floats), identical picks, slower. */
int ptt_fps_ws_f32(const float* xyz, int B, int N, int npoint, int32_t* idx_out, float* workspace,
                   size_t workspace_elems, ptt_stream_t stream);

/* ---------------------------------------------------------------------------------
 * F1b (ABI 29)  feature-space furthest point sampling (3DSSD's F-FPS)
 * stands in for _ext.furthest_point_sampling_with_dist(square_distance(cat, cat), npoint) of sample_method 'ffps'
 * (pointnet2_modules.py:64-67, cat = [xyz ; features] per point), which the reference's extension never provided —
 * without the (B,N,N) matrix or the (B,N,N,C+3) intermediate it is the sum of: the distances are formed on the fly.
 *   xyz (B,N,3) f32 contiguous; feat: element [b,c,k] at feat[b*feat_sb + c*feat_sc + k*feat_sn] (element strides: a (B,C,N)
 *   tensor, the point-major (B,N,C) rows of the fused path and rows with a padded stride are all read in place)
 *   -> idx_out (B,npoint) i32
 * With v_k = [x_k, y_k, z_k, f_0k, ..., f_(C-1)k] and D = C + 3: d(i,k) is an fp32 accumulator that starts at 0 and takes, for
 * c = 0 .. D-1 in this order, t = v_i[c] - v_k[c]; acc = acc + t*t — every operation rounded on its own, no FMA contraction.
 * tmp[:] = 1e10, idx[0] = 0; for j = 1 .. npoint-1: tmp[k] = min(tmp[k], d(idx[j-1], k)) for every k, idx[j] = the lowest
 * k that attains max tmp. No origin-ball skip (that is ptt_fps_f32's, inherited from the coordinate op): with C == 0
 * (feat may be NULL) the picks are those of this definition, not ptt_fps_f32's. A cloud of identical points gives zeros.
 * Non-finite input is outside the contract; no index leaves [0, N) even then.
 * Limits (PTT_EUNSUPPORTED beyond them): N <= 16384, C <= 1024, npoint <= 15360 (npoint > N is allowed), and one cloud's
 * features within 2^31 elements: (N-1)*|feat_sn| + (C-1)*|feat_sc| <= INT_MAX. Null xyz / idx_out (feat with C > 0) or
 * B, N, npoint < 1 or C < 0: PTT_EINVAL. Both are answered before any runtime call.
 * One workgroup per cloud. C = 128 / 256 / 257 with N <= 512 / 256 / 256 (the model's levels): every point's vector stays in its
 * thread's registers; any other shape streams the cloud's N x D values from L2 every iteration (coalesced when feat_sn == 1).
 * Same picks either way. No workspace, no allocation, no host synchronisation, capturable.
 * ------------------------------------------------------------------------------- */
int ptt_ffps_f32(const float* xyz, const float* feat, int64_t feat_sb, int64_t feat_sc, int64_t feat_sn,
                 int B, int N, int C, int npoint, int32_t* idx_out, ptt_stream_t stream);

/* ---------------------------------------------------------------------------------
 * F2  gather centres
 * replaces _ext.gather_points(features, idx)                pointnet2_utils.py:112
 *          _ext.gather_points_grad(grad_out, idx, N)        pointnet2_utils.py:118
 *   feat (B,C,N) f32, idx (B,M) i32 -> out (B,C,M);   out[b,c,j] = feat[b,c,idx[b,j]]
 *   grad: grad_feat (B,C,N) is zero-filled by the call, then += over all j.
 * ------------------------------------------------------------------------------- */
int ptt_gather_f32(const float* feat, const int32_t* idx, int B, int C, int N, int M,
                   float* out, ptt_stream_t stream);
int ptt_gather_grad_f32(const float* grad_out, const int32_t* idx, int B, int C, int N,
                        int M, float* grad_feat, ptt_stream_t stream);

/* Centres of one SA level in one launch (the xyz gather + transposes of pointnet2_modules.py:79-81 and
 * the int64 cast of :90): new_xyz[b,m,:] = xyz[b, idx[b,m], :]; idx == NULL selects the first M points
 * ('sequence' sampling, :70-71); idx64_out (B,M) receives the indices as int64, or NULL. */
int ptt_select_centres_f32(const float* xyz, const int32_t* idx, int B, int N, int M, float* new_xyz,
                           int64_t* idx64_out, ptt_stream_t stream);

/* ---------------------------------------------------------------------------------
 * F3  ball query  (centres first, as the reference calls it)
 * replaces _ext.ball_query(new_xyz, xyz, radius, nsample)   pointnet2_utils.py:287
 *   new_xyz (B,M,3), xyz (B,N,3) -> idx_out (B,M,nsample) i32
 * first `nsample` indices k in ascending order with (dx*dx+dy*dy)+dz*dz < r*r
 * (fp32, strict); unfilled slots repeat the first hit; no hit -> zeros.
 * ------------------------------------------------------------------------------- */
int ptt_ball_query_f32(const float* new_xyz, const float* xyz, int B, int M, int N,
                       float radius, int nsample, int32_t* idx_out, ptt_stream_t stream);

/* ptt_select_centres_f32 + ptt_ball_query_f32 of one SA level in one launch (same results): new_xyz (B,M,3), idx64_out
 * (B,M) or NULL, idx_out (B,M,nsample); sel (B,M) int32 sample indices or NULL for the first M points. */
int ptt_centres_ball_query_f32(const float* xyz, const int32_t* sel, int B, int N, int M, float radius, int nsample,
                               float* new_xyz, int64_t* idx64_out, int32_t* idx_out, ptt_stream_t stream);

/* ---------------------------------------------------------------------------------
 * F4  grouping
 * replaces _ext.group_points(features, idx)                 pointnet2_utils.py:237
 *          _ext.group_points_grad(grad_out, idx, N)         pointnet2_utils.py:257
 *   feat (B,C,N), idx (B,M,ns) -> out (B,C,M,ns);  out[b,c,j,k] = feat[b,c,idx[b,j,k]]
 * ------------------------------------------------------------------------------- */
int ptt_group_f32(const float* feat, const int32_t* idx, int B, int C, int N, int M,
                  int ns, float* out, ptt_stream_t stream);
int ptt_group_grad_f32(const float* grad_out, const int32_t* idx, int B, int C, int N,
                       int M, int ns, float* grad_feat, ptt_stream_t stream);

/* ---------------------------------------------------------------------------------
 * N3  deterministic scatter-add: the backward of gather_points (E = M) and group_points (E = M*nsample)
 * replaces _ext.gather_points_grad / _ext.group_points_grad   pointnet2_utils.py:118,257
 *   out[b,c,n] = sum of src[b,c,e] over the entries e with idx[b,e] == n, added in ascending e, i.e. the
 *   result of the sequential loop — bit-identical run to run (upstream's atomicAdd kernels are not).
 *   idx (B,E) i32 in [0,N); src (B,C,E); out (B,C,N); E <= 16384.
 *   workspace: ptt_scatter_add_det_workspace(B,N,E) bytes of device memory (PTT_EWORKSPACE if smaller).
 * ------------------------------------------------------------------------------- */
size_t ptt_scatter_add_det_workspace(int B, int N, int E);
int ptt_scatter_add_det_f32(const float* src, const int32_t* idx, int B, int C, int N, int E, float* out,
                            void* workspace, size_t workspace_bytes, ptt_stream_t stream);

/* ---------------------------------------------------------------------------------
 * T1  k nearest neighbours inside one cloud
 * replaces square_distance(xyz, xyz).argsort()[:, :, :k]    transformer_block/variants.py:150-151
 *   xyz (B,N,3) -> idx_out (B,N,k) i32, ascending by (squared distance, index);
 *   d = (dx*dx+dy*dy)+dz*dz in fp32 (model_utils/layer_utils.py:26). Requires k <= N.
 * ------------------------------------------------------------------------------- */
int ptt_knn_f32(const float* xyz, int B, int N, int k, int32_t* idx_out,
                ptt_stream_t stream);
/* Same, additionally writing rel_out (B,N,k,3) = xyz_i - xyz_neighbour, the input of fc_delta
 * (variants.py:158 `xyz[:, :, None] - knn_xyz`): the pair kernel then starts without a dependent
 * index -> coordinate round trip. rel_out may be NULL. */
int ptt_knn_rel_f32(const float* xyz, int B, int N, int k, int32_t* idx_out, float* rel_out,
                    ptt_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Weight packing for the fp32-MFMA kernels.
 *   W (Cout,K) row-major (an nn.Linear / 1x1-conv weight)  ->  packed fragment order
 *   [K8][Cout32][64 lanes][4]  with K padded to a multiple of 8 and Cout to 32 (zeros).
 * ------------------------------------------------------------------------------- */
size_t ptt_packed_weight_elems(int Cout, int K);
int ptt_pack_weight_f32(const float* W, int Cout, int K, float* packed,
                        ptt_stream_t stream);
/* Same, with the input channels rotated: packed position k holds original channel (k+rot) mod K.
 * The fused SA kernel keeps each grouped row as [features | xyz] (16-byte aligned feature rows),
 * while the reference concatenates [xyz | features] (pointnet2_utils.py:359-361): pack the FIRST
 * SharedMLP layer of ptt_sa_fused_fwd_f32 with rot = 3 when use_xyz, rot = 0 otherwise. */
int ptt_pack_weight_rot_f32(const float* W, int Cout, int K, int rot, float* packed,
                            ptt_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Row-wise linear layer on fp32 MFMA:  out = act(X @ W^T * scale + shift) (+ residual)
 * replaces nn.Linear / Conv1d(k=1) forwards on the hot path:
 *   TransformerBlock.fc1 / w_qs / w_ks / w_vs / fc2          variants.py:154-156,164
 *   PointNet2BackboneLight.cov_final                         pointnet2_backbone.py:46
 *   X (rows, K) with row stride ldx; out (rows, Cout) with row stride ldo;
 *   scale/shift per output channel (NULL = 1 / 0); residual (rows, Cout) stride ldr or NULL.
 * ------------------------------------------------------------------------------- */
int ptt_linear_f32(const float* X, int rows, int K, int ldx, const float* Wpacked, int Cout,
                   const float* scale, const float* shift, int relu, const float* residual,
                   int ldr, float* out, int ldo, ptt_stream_t stream);

/* ---------------------------------------------------------------------------------
 * F4+F5+F6+F7 fused: group -> (xyz - centre)/radius -> concat -> SharedMLP(eval BN
 * folded to scale/shift, ReLU) -> max over nsample.
 * replaces QueryAndGroup.forward                           pointnet2_utils.py:320-380
 *          SharedMLP forward (eval)                        pytorch_utils.py:12-36
 *          F.max_pool2d over nsample                       pointnet2_modules.py:85-88
 * Grouped tensors never reach HBM.
 * ------------------------------------------------------------------------------- */
#define PTT_SA_MAX_LAYERS 4

typedef struct ptt_sa_layer {
    const float* Wpacked; /* packed (Cout,Cin) conv weight; layer 0: rot = 3 if use_xyz      */
    const float* scale;   /* (Cout) gamma/sqrt(var+eps), or NULL = 1                   */
    const float* shift;   /* (Cout) beta - mean*scale (or conv bias), or NULL = 0      */
    int Cin;              /* input channels of this layer (first layer: 3*use_xyz + C) */
    int Cout;             /* multiple of 32, <= 256 (PTT_EUNSUPPORTED otherwise)       */
    int relu;
} ptt_sa_layer;

/* A stack of up to PTT_SA_MAX_LAYERS 1x1 convolutions (+ folded BatchNorm + ReLU) over point rows in one launch:
 * out = L_n(... L_1(X)) (+ residual). Replaces the eval-mode Conv1d stacks of the heads
 * (voting_heads/centroids_voting_head.py: vote_layer, cla_layer; voting_heads/box_voting_head.py: refine_layer) and the
 * two trailing convolutions of CosineSimAug (similarity_modules/p2b_xcoor.py:43-45), which the reference runs as one
 * cuDNN convolution + batch_norm + relu per layer. X (rows, K <= 264) with row stride ldx; inner layers Cout <= 256, the
 * last layer any Cout <= 384 (e.g. 1, 5, 259); layers[i].Wpacked from ptt_pack_weight_f32, scale NULL when the BatchNorm
 * scale is folded into the weights (one instruction less per value in the epilogue). */
int ptt_rows_mlp_f32(const float* X, int rows, int K, int ldx, const ptt_sa_layer* layers, int n_layers,
                     const float* residual, int ldr, float* out, int ldo, ptt_stream_t stream);

/* Point jobs (round 4): the centre selections + ball queries of several set-abstraction levels and one kNN in ONE launch — the
 * index ops between the level-0 furthest point sampling and the first SharedMLP of one tracklet frame
 * (pointnet2_modules.py:68-83 for three levels, transformer_block/variants.py:150-151). Every job reads the RAW clouds
 * xyz (B,Nraw,3): centre m of cloud b is raw[centre_sel[b][m]] (NULL: raw[m]), point k is raw[point_sel[b][k]] (NULL:
 * raw[k]), k < Npts; with 'sequence' sampling above level 0 both selections of every level are prefixes of the level-0
 * sample indices, so the levels do not depend on each other.
 *   kind 0  ball query: new_xyz (B,M,3), idx64_out (B,M) = the centres' raw indices or NULL, idx_out (B,M,nsample) = positions
 *           k inside the level's points — the results of ptt_centres_ball_query_f32 on the level's own point tensor;
 *   kind 1  kNN of the Npts <= 128 points among themselves (M == Npts): idx_out (B,Npts,nsample), rel_out (B,Npts,nsample,3)
 *           or NULL — the results of ptt_knn_rel_f32 on the points' own tensor. */
/* F3 for large clouds (round 5): the same results as ptt_ball_query_f32 / ptt_centres_ball_query_f32 through a uniform grid —
 * the cloud's points binned into cells of edge >= 1.001 radius, a centre tests the points of its 27 neighbouring cells only, the
 * first nsample hits IN INDEX ORDER restored by a bitmap (bit-identical to the sweep). workspace: ptt_ball_query_grid_workspace(B, N)
 * bytes, 16-byte aligned (PTT_EWORKSPACE if smaller); N <= 131072. Worth it from a few thousand points per cloud on. */
size_t ptt_ball_query_grid_workspace(int B, int N);
int ptt_ball_query_grid_f32(const float* new_xyz, const float* xyz, int B, int M, int N, float radius, int nsample,
                            int32_t* idx_out, void* workspace, size_t workspace_bytes, ptt_stream_t stream);
int ptt_centres_ball_query_grid_f32(const float* xyz, const int32_t* sel, int B, int N, int M, float radius, int nsample,
                                    float* new_xyz, int64_t* idx64_out, int32_t* idx_out, void* workspace, size_t workspace_bytes,
                                    ptt_stream_t stream);
/* One launch for a small FPS-sampled set-abstraction level whose centres then meet in a TransformerBlock (vote_aggregation +
 * the box head's transformer at one tracklet frame, box_voting_head.py:75-86): ptt_fps_f32 + ptt_centres_ball_query_f32 +
 * ptt_knn_rel_f32 (of the CENTRES among themselves) with identical results. xyz (B,N<=256,3) -> inds (B,M) i32, inds64 (B,M)
 * or NULL, new_xyz (B,M,3), idx (B,M,nsample), knn (B,M,k) + rel (B,M,k,3) (k = 0: neither). M <= 128. */
int ptt_fps_ball_knn_f32(const float* xyz, int B, int N, int M, float radius, int nsample, int k, int32_t* inds,
                         int64_t* inds64, float* new_xyz, int32_t* idx, int32_t* knn, float* rel, ptt_stream_t stream);
#define PTT_POINT_JOBS_MAX 4
typedef struct ptt_point_job {
    const float* xyz; const int32_t* centre_sel; const int32_t* point_sel;
    float* new_xyz; int64_t* idx64_out; int32_t* idx_out; float* rel_out;
    int32_t kind, sel_ld, B, Nraw, Npts, M, nsample;
    float radius;
} ptt_point_job;
int ptt_point_jobs_f32(const ptt_point_job* jobs, int n_jobs, ptt_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Row jobs (round 4): up to PTT_ROW_JOBS_MAX independent row-wise layers in ONE launch, each
 *     out = act(A @ W^T * scale + shift) (+ residual)
 * with the operand A formed while it is staged and the result consumed in the epilogue — the launch
 * chain of ONE tracklet frame (tools/eval_utils/eval_tracking_utils.py:140-152: B = 1) is ~45 dependent
 * launches of 128-2048 rows, each a few microseconds of work behind ~5 us of launch latency, so what
 * counts is how many launches are on the chain. One job replaces one of
 *   nn.Linear / Conv1d(k=1) forwards (transformer_block/variants.py:154-164; voting_heads/
 *     centroids_voting_head.py:83-94 cla_layer / vote_layer; box_voting_head.py:88-90 refine_layer;
 *     similarity_modules/p2b_xcoor.py:43-45; pointnet2_backbone.py:46),
 * and the element-wise code around them:
 *   prologue 0  A = [X | X2]: the columns [0,K1) from X (row stride ldx), [K1,K) from X2 (ldx2) — the
 *               torch.cat((xyz, feats)) in front of vote_layer (centroids_voting_head.py:86-90) and of
 *               CosineSimAug's per-template-point term without the copy (weights packed with the
 *               matching input-channel rotation);
 *   prologue 1  A[r,:] = relu(fc_delta[0](rel[r,:]))            variants.py:158 (first Linear + ReLU; w1 (K,4) =
 *               [wx wy wz bias] per channel), so that fc_delta is one launch;
 *   prologue 2  A[(i,j),:] = q_i - k[knn_ij] + pos_ij            variants.py:160 (argument of fc_gamma);
 *   epilogue 1  res_i = sum_j softmax_j(y_ij * sm_scale) * (v[knn_ij] + pos_ij)   variants.py:161-163 — the 32 rows
 *               of a tile are the 16 neighbours of two points, so the softmax over neighbours is local to the
 *               accumulator tile (the per-column bias cancels and is not read); out (points, Cout).
 *   prologue 3  A[(c,j),:] = act0(term[idx_cj,:] + Wx . (xyz[idx_cj] - centre_c)(/radius)): the grouped input of a
 *               set-abstraction level whose first convolution is hoisted to one row per POINT (ptt_sa_desc.l0_point_term;
 *               QueryAndGroup + SharedMLP layer 0, pointnet2_utils.py:320-361, pytorch_utils.py:12-36): X = term
 *               (B*N rows, ldx), idx (B,M,ns) from the ball query, wx (3,K), act0 = ReLU when pro_relu;
 *   epilogue 2  out[c,:] = act(max_j y_cj): the max-pool over the ns = 16 or 32 neighbours of a centre
 *               (F.max_pool2d, pointnet2_modules.py:85-87), local to the 32-row accumulator tile; out (B*M, Cout).
 *               Prologue 3 -> layer 1, then a plain layer with epilogue 2 = vote_aggregation (box_voting_head.py:75-79) in two
 *               launches of 1024 rows over the chip, where the fused SA kernel is 16 workgroups at one frame.
 *   act         0 none, 1 ReLU, 2 sigmoid (`raw`, if given, receives the value before the activation:
 *               pred_centroids_cls beside its sigmoid, centroids_voting_head.py:84,92-94)
 *   residual    out column c >= res_split adds res[row*ldr + c - res_split], c < res_split adds
 *               res2[row*ldr2 + c] (either may be NULL): `vote_in + vote_layer(vote_in)` with vote_in = cat(xyz, feats)
 *               (centroids_voting_head.py:90), `offsets[:, 0:3] + centres` (box_voting_head.py:91);
 *   output      column c >= out_split goes to out[row*ldo + c - out_split + out_col0], c < out_split to
 *               out2[row*ldo2 + c]: the slices / concatenations behind the heads (votes vs. votes_feats).
 * A workgroup of 8 waves owns a 32-row x (32 * col_tiles)-column tile and splits K over 8 / col_tiles wave groups
 * (partial sums meet in LDS): a 128-row layer is 64-192 workgroups with a 1-2 us MFMA chain each instead of 16 with 7 us.
 * Wpacked from ptt_pack_weight_f32 (K <= 1024). Jobs of one launch must not depend on each other.
 * ------------------------------------------------------------------------------- */
#define PTT_ROW_JOBS_MAX 4
typedef struct ptt_row_job {
    const float* X; const float* X2;
    const float* Xmax;                                 /* prologue 0, optional: A = max(X, Xmax) element-wise (same rows / stride as X; needs
                                                          K1 == K, K % 4 == 0, 16-byte aligned rows): the two halves of the split ptt_xcorr_fused_fwd_f32 */
    const float* Wpacked; const float* scale; const float* shift;
    const float* res; const float* res2;
    float* out; float* out2; float* raw;
    const float* rel; const float* w1;                 /* prologue 1: (rows,3), (K,4) */
    const float* qkv; const int32_t* knn; const float* pos;   /* prologue 2 / epilogue 1: (points, ldq) rows holding q | k | v at
                                                          column offsets q_off / k_off / v_off, (points,16) neighbour indices
                                                          inside the point's cloud of N points, (rows, ldp) positional term */
    int32_t rows, K, K1, ldx, ldx2, Cout;
    int32_t act, res_split, ldr, ldr2, out_split, out_col0, ldo, ldo2, ldraw;
    int32_t prologue, epilogue, ldq, q_off, k_off, v_off, ldp, N;
    float sm_scale;
    int32_t col_tiles;                                 /* 0: the library picks 1, 2 or 4 by launch size */
    const int32_t* idx; const float* xyz; const float* centres; const float* wx;   /* prologue 3 */
    float radius;
    int32_t ns, M, normalize_xyz, pro_relu;            /* prologue 3 / epilogue 2: neighbours per centre, centres per cloud */
} ptt_row_job;
int ptt_row_jobs_f32(const ptt_row_job* jobs, int n_jobs, ptt_stream_t stream);

typedef struct ptt_sa_desc {
    const float* xyz;     /* (B,N,3)                                                   */
    const float* new_xyz; /* (B,M,3) centres                                           */
    const int32_t* idx;   /* (B,M,nsample) from ptt_ball_query_f32                     */
    const float* feat;    /* point features or NULL when C == 0                        */
    int64_t feat_sb, feat_sc, feat_sn; /* element strides of feat[b][c][n]             */
    float* out;           /* pooled features                                           */
    int64_t out_sb, out_sc, out_sm;    /* element strides of out[b][c][m]              */
    int B, N, M, nsample, C;           /* nsample 16, 32 or 64 (PTT_EUNSUPPORTED otherwise) */
    float radius;
    int use_xyz;          /* prepend the 3 relative coordinates (reference default); with C == 0 it must be 1:
                           * a level needs the coordinates or point features (PTT_EINVAL otherwise) */
    int normalize_xyz;    /* divide them by radius (pointnet2_utils.py:353-354)        */
    int n_layers;
    ptt_sa_layer layers[PTT_SA_MAX_LAYERS];
    /* Optional: layer 0 of the SharedMLP hoisted out of the grouped stage. The first Conv2d is linear in
     * [rel ; f_n], so  layer0(centre i, neighbour n) = act(T[b][n][:] + Wx . rel(i,n))  with
     *   T  = scale0 * (W0[:,3:] . f_n) + shift0     one row per POINT (ptt_linear_f32), (B,N,C0) contiguous
     *   Wx = (scale0 * W0[:, 0:3])^T                (3,C0)
     * which moves 2*C*C0 flop per grouped row (N*... rows instead of M*nsample) out of the kernel.
     * When l0_point_term != NULL: use_xyz must be 1 (PTT_EINVAL otherwise), feat/C are ignored and `layers` holds the REMAINING layers
     * (layers[0].Cin == l0_channels). NULL = layer 0 runs inside the kernel on the gathered rows. */
    const float* l0_point_term;
    const float* l0_xyz_weight;
    int l0_channels;
    int l0_relu;
    /* Optional (ABI 22; the stream shape ABI 26): workspace of at least ptt_sa_compact_workspace(B, M) bytes, 16-byte
     * aligned (PTT_EWORKSPACE otherwise). Non-NULL: two extra launches first reduce every ball to its DISTINCT rows, padded
     * to a class size c in {4, 8, 16, 32}, and the MLP runs on tiles of whole balls of one class. The max over a multiset
     * equals the max over its distinct members: the output is bitwise the dense one. Two shapes honour it:
     *   - the level without point features (C == 0, use_xyz, nsample 32, 3 -> 64 -> 64 -> 128, the SA0 shape), 32 / c balls
     *     per 32-row tile. Distinct = first occurrence of an (x,y,z) bit pattern among the ball's slots: a ball's padding
     *     slots repeat its first hit, and neighbours with bit-identical coordinates give bit-identical rows;
     *   - the stream shape (l0_point_term with 128 channels, then 128 -> 128 -> 256, nsample 32, no per-layer scale),
     *     64 / c balls per 64-row tile. Distinct = real hit: slot s is kept iff s == 0 or idx[s] != idx[0]. A row carries
     *     its neighbour's feature row, so no coordinate is compared; "distinct rows per ball" below is the real-hit count.
     * Ignored by the other shapes; NULL = every one of the nsample rows (the dense path). idx is not modified. Worth its two
     * launches only where most slots are padding and the launch is large (ptt_amd gates it on B * M).
     * Layout (int32 words, T = B*M; read by tests, not an interface to build on):
     *   [0, 4)                 balls per class (c = 4, 8, 16, 32), [4, 16) reserved
     *   [16, 16+T)             distinct rows per ball
     *   [16+T+k*T, +T)         the balls (b*M + m) of class k, in any order (first n_k entries)
     *   [16+5T+(c_k-4)*T, +c_k*T)  their rows: ball at list position q owns entries [q*c_k, (q+1)*c_k) — its distinct
     *                          neighbour indices in slot order, then the first one repeated */
    void* compact_ws;
    size_t compact_ws_bytes;
} ptt_sa_desc;

int ptt_sa_fused_fwd_f32(const ptt_sa_desc* d, ptt_stream_t stream);
size_t ptt_sa_compact_workspace(int B, int M);

/* ---------------------------------------------------------------------------------
 * N1  P2B cosine-similarity feature augmentation, fused
 * replaces CosineSimAug.forward up to the max over the template axis
 *                                              similarity_modules/p2b_xcoor.py:25-42
 *   fusion[b,:,i,j] = [cos(templ_i, search_j) | templ_xyz_i | templ_feat_i]  (never materialised)
 *   out[b,:,j] = max_i SharedMLP(fusion)[b,:,i,j]
 * Layer 0 is split: W0.fusion = w_sim*cos_ij + P[b,i,:], with P = W0[:,1:].[xyz_i;feat_i] computed
 * once per template point by ptt_linear_f32. `layers` are the REMAINING SharedMLP layers.
 * The template seeds are walked in chunks of 64 with a running max (Nt % 64 == 0, PTT_EUNSUPPORTED otherwise); the cosine map comes from
 * ptt_cosine_map_f32 (below).
 * ------------------------------------------------------------------------------- */
typedef struct ptt_xcorr_desc {
    const float* cos_t;                 /* (B,Ns,Nt) cosine map cos(search_j, templ_i) from ptt_cosine_map_f32 (one launch
                                           per batch: computing it inside every workgroup cost ~340 vector-ALU / load
                                           instructions per wave beside the other workgroup's MFMA stream)             */
    const float* P;                     /* (B,Nt,C0) contiguous, see above                   */
    const float* w_sim;                 /* (C0) W0[:,0]                                      */
    const float* scale0;                /* (C0) folded BN of layer 0 (NULL = 1 / 0)          */
    const float* shift0;
    float* out;                         /* out[b][c][j], element strides below               */
    int64_t out_sb, out_sc, out_sn;
    float* sim_out;                     /* optional (B,Nt,Ns) copy of the cosine map in the reference's orientation, or NULL */
    int B, Ns, Nt, C0;
    int n_layers;
    ptt_sa_layer layers[PTT_SA_MAX_LAYERS];
    /* Split form, for a handful of frames (round 4; B * Ns search points would be as many workgroups: half the chip at one
     * frame): split != 0 launches TWO workgroups per search point, each with half of the template points, and forms the
     * cosines inside the kernel (cos_t is not read, ptt_cosine_map_f32 not needed). Half h writes its maxima to
     * out + h * out_sh (same strides); the maximum over the template axis is the element-wise maximum of the two, taken by
     * the consumer (ptt_row_job.Xmax). search_feat[b][j][:], templ_feat[b][i][:] with unit channel stride, element strides
     * s_sb / s_sn / t_sb / t_sn, C channels (C % 4 == 0), eps of F.cosine_similarity; B * Ns % 8 == 0; sim_out NULL
     * (PTT_EINVAL otherwise). */
    int32_t split; int64_t out_sh;
    const float* search_feat; const float* templ_feat;
    int64_t s_sb, s_sn, t_sb, t_sn;
    int C; float eps;
} ptt_xcorr_desc;

int ptt_xcorr_fused_fwd_f32(const ptt_xcorr_desc* d, ptt_stream_t stream);

/* cos_t[b][j][i] = <templ_i, search_j> / (max(|templ_i|, eps) * max(|search_j|, eps))   (F.cosine_similarity, p2b_xcoor.py:35-36)
 * search_feat[b][n][c] / templ_feat[b][i][c] with element strides; cos_t (B,Ns,Nt) contiguous. */
int ptt_cosine_map_f32(const float* search_feat, int64_t s_sb, int64_t s_sn, int64_t s_sc, const float* templ_feat,
                       int64_t t_sb, int64_t t_sn, int64_t t_sc, int B, int Ns, int Nt, int C, float eps,
                       float* cos_t, ptt_stream_t stream);

/* ---------------------------------------------------------------------------------
 * T2..T6 fused per-(point,neighbour) part of the Point-Transformer block:
 *   delta = fc_delta(xyz_i - xyz_j);  a = fc_gamma(q_i - k_j + delta);
 *   attn = softmax_j(a / sqrt(D));    res_i = sum_j attn * (v_j + delta)
 * replaces TransformerBlock.forward lines                  variants.py:158-163
 *   qkv (B,N,3*D) = [q | k | v] rows (from ptt_linear_f32 with the stacked weight),
 *   knn (B,N,k) i32. One head (heads 0 or 1): D 128, 256 or 512 and k 8, 16 or 32 are instantiated; several heads (2, 4, 8 with
 *   D / heads >= 32, one 32-column MFMA tile): D 128 or 256 and k 8, 16 or 32, D = 512 and k = 16 only — so heads 2, 4 at D 128,
 *   heads 2, 4, 8 at D 256 and 512 (PTT_EUNSUPPORTED otherwise). A 32-row tile holds 32 / k whole points of one cloud, so N % (32 / k) == 0:
 *   at k = 8, N must be a multiple of 4; at k = 16, N must be even (a tile holds two points of
 *   one cloud; PTT_EUNSUPPORTED otherwise); at k = 32 any N. N >= k. A refused launch (PTT_EUNSUPPORTED) writes nothing.
 *   res (B,N,D); attn (B,N,k,D) or NULL (the heads discard it: centroids_voting_head.py:76).
 * ------------------------------------------------------------------------------- */
typedef struct ptt_attn_desc {
    const float* xyz;      /* (B,N,3) */
    const float* rel;      /* (B,N,k,3) from ptt_knn_rel_f32, or NULL (computed from xyz and knn) */
    const int32_t* knn;    /* (B,N,k) */
    const float* qkv;      /* (B,N,3*D) */
    const float* Wd1p;     /* packed (ptt_pack_weight_f32, K = 4) [fc_delta[0].weight (D,3) | fc_delta[0].bias (D)]:
                              layer 0 of the position encoding runs as one MFMA K-block on rows [rel.xyz 1]   */
    const float* Wd2p;     /* packed fc_delta[2].weight */
    const float* bd2;
    const float* Wg1p;     /* packed fc_gamma[0].weight */
    const float* bg1;
    const float* Wg2p;     /* packed fc_gamma[2].weight */
    const float* bg2;      /* fc_gamma[2].bias: accepted, never read — a per-channel constant over the
                              neighbours cancels in softmax_j                                               */
    float* res;            /* (B,N,D) */
    float* attn;           /* (B,N,k,D) or NULL */
    int B, N, k, D;
    const int32_t* order;  /* (B,N) from ptt_spatial_order_f32, or NULL: which flat point (b*N + n) launch slot s works on. A
                              permutation inside every cloud; results do not depend on it (L2 locality of the k | v gathers) */
    int heads;             /* 0 or 1: TransformerBlock. 2, 4, 8: MulHeadTransformerLayer (multitransformer.py:11-63) with
                              hd = D / heads >= 32 (D 128: heads 2, 4; D 256: 2, 4, 8, any instantiated k; D 512: 2, 4, 8 at
                              k = 16): Wg1p / Wg2p are the packed hd x hd fc_gamma weights that every head shares, bg1
                              is fc_gamma[0].bias repeated `heads` times (D floats), the softmax scale is 1 / sqrt(hd), and
                              attn is written in the reference's (B*heads, N, k, hd) layout                                  */
} ptt_attn_desc;

int ptt_pt_attn_pair_f32(const ptt_attn_desc* d, ptt_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Split-bf16 form of the single-head pair kernel (ABI 37; TransformerBlock.precision = 'bf16x2', off by default).
 * Every fp32 operand x of the three D x D GEMMs (fc_delta[2], fc_gamma[0], fc_gamma[2]) is taken as two bf16 pieces,
 *   hi = bf16(x) rounded to nearest even, lo = bf16(x - float(hi)),
 * and a product is hi.hi + hi.lo + lo.hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation. Everything else — rel rows,
 * fc_delta[0], q | k | v, biases, softmax, the weighted sum, res and attn — is the fp32 kernel's.
 *
 * Split pack of a (Cout, K) fp32 weight W (row-major, W[col][k]), Cout % 32 == 0 and K % 16 == 0 (PTT_EINVAL otherwise):
 * 2 * Cout * K bf16 elements (uint16 words), NT = Cout / 32. Element
 *     e = (((kb * NT + ct) * 2 + piece) * 64 + lane) * 8 + j,   kb < K / 16, ct < NT, piece < 2, lane < 64, j < 8
 * holds piece `piece` (0 = hi, 1 = lo) of W[32 * ct + (lane & 31)][16 * kb + 8 * (lane >> 5) + j]: the B-fragment order of
 * v_mfma_f32_32x32x16_bf16, each lane's fragment of a (16-channel block, 32-column tile, piece) being one 16-byte load.
 * ptt_split_weight_elems is a host call (no device work): the bf16 elements of one split pack, both pieces; 0 for sizes that
 * are not positive. */
int ptt_split_weight_elems(int Cout, int K);
int ptt_pack_weight_split_bf16(const float* W, int Cout, int K, void* out, ptt_stream_t stream);

/* ptt_attn_desc without `heads`: one head. The shape rules and refusals of ptt_pt_attn_pair_f32 for one head: D 128, 256, 512
 * and k 8, 16, 32 are instantiated, N % (32 / k) == 0 and N >= k (PTT_EUNSUPPORTED otherwise). A refused launch writes nothing. */
typedef struct ptt_attn_split_desc {
    const float* xyz;      /* (B,N,3) */
    const float* rel;      /* (B,N,k,3) from ptt_knn_rel_f32, or NULL */
    const int32_t* knn;    /* (B,N,k) */
    const float* qkv;      /* (B,N,3*D) fp32 */
    const float* Wd1p;     /* the fp32 pack of ptt_attn_desc.Wd1p: fc_delta[0] stays one exact fp32 K-block */
    const void* Wd2s;      /* split pack of fc_delta[2].weight */
    const float* bd2;
    const void* Wg1s;      /* split pack of fc_gamma[0].weight */
    const float* bg1;
    const void* Wg2s;      /* split pack of fc_gamma[2].weight */
    const float* bg2;      /* accepted, never read (cancels in softmax_j) */
    float* res;            /* (B,N,D) */
    float* attn;           /* (B,N,k,D) or NULL */
    int B, N, k, D;
    const int32_t* order;  /* (B,N) from ptt_spatial_order_f32, or NULL; results do not depend on it */
} ptt_attn_split_desc;

int ptt_pt_attn_pair_split_f32(const ptt_attn_split_desc* d, ptt_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Split-bf16 form of the streamed set-abstraction level (ABI 38; PointnetSAModuleVotes.precision = 'bf16x2', off by default).
 * One shape, the one ptt_sa_fused_fwd_f32 hands to its streamed kernel: a hoisted layer 0 with 128 channels, kernel layer 1
 * 128 -> 128 with ReLU, kernel layer 2 128 -> 256 (ReLU when relu2 != 0), 32 neighbours, the BatchNorm scale folded into the
 * weights, fp32 shifts. h0 = act(l0_point_term[idx] + l0_xyz_weight . rel) is formed in fp32 exactly as ptt_sa_fused_fwd_f32
 * forms it (the normalize_xyz divide, the l0_relu floor), then split into hi = bf16(x) (round to nearest even) and
 * lo = bf16(x - float(hi)); each layer takes hi.hi + hi.lo + lo.hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation, the
 * shifts, the ReLUs and the max over the 32 neighbours run in fp32 (h1 is split again before layer 2), the store is fp32.
 * W1s / W2s: ptt_pack_weight_split_bf16 of the (128,128) and (256,128) weights with the scale folded in. shift1 / shift2 may
 * be NULL (no shift). B == 0 or M == 0: PTT_OK, nothing is launched. A NULL pointer among the others: PTT_EINVAL;
 * l0_point_term, l0_xyz_weight, W1s or W2s not 16-byte aligned, or a negative output stride: PTT_EINVAL; an array of the
 * launch over 2 GiB (32-bit offsets): PTT_EUNSUPPORTED. A refused call writes nothing. */
typedef struct ptt_sa_split_desc {
    const float* xyz;            /* (B,N,3) */
    const float* new_xyz;        /* (B,M,3) */
    const int32_t* idx;          /* (B,M,32) neighbour indices in [0,N) */
    const float* l0_point_term;  /* (B,N,128): layer 0's feature half per point, shift included */
    const float* l0_xyz_weight;  /* (3,128): layer 0's coordinate columns, transposed, scale folded */
    int l0_relu;                 /* layer 0's ReLU */
    const void* W1s;             /* split pack, Cout = 128, K = 128 */
    const float* shift1;         /* (128) or NULL */
    const void* W2s;             /* split pack, Cout = 256, K = 128 */
    const float* shift2;         /* (256) or NULL */
    int relu2;                   /* layer 2's ReLU (after the max, which commutes with it) */
    float* out;                  /* element (b, c, m) at out[b*out_sb + c*out_sc + m*out_sm] */
    long long out_sb, out_sc, out_sm;
    int B, N, M;
    float radius;
    int normalize_xyz;
} ptt_sa_split_desc;

int ptt_sa_stream_split_f32(const ptt_sa_split_desc* d, ptt_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Split-bf16 form of the fused CosineSimAug kernel (ABI 39; CosineSimAug.precision = 'bf16x2', off by default).
 * One shape, the shipped configuration's MLP.CHANNELS = [260, 256, 256, 256] on the batched form of ptt_xcorr_fused_fwd_f32
 * (cos_t given, no split): C0 = 256 with the BatchNorm of layer 0 folded into P and w_sim, kernel layer 1 256 -> 256 with ReLU,
 * kernel layer 2 256 -> 256 (ReLU when relu2 != 0), the BatchNorm scale folded into the weights, fp32 shifts, Nt % 64 == 0
 * walked in chunks of 64 with a running max. h0 = max(P[b,i,:] + w_sim * cos_t[b,j,i], 0) is formed in fp32 exactly as
 * ptt_xcorr_fused_fwd_f32 forms it, then split into hi = bf16(x) (round to nearest even) and lo = bf16(x - float(hi)); each
 * layer takes hi.hi + hi.lo + lo.hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation, the shifts, layer 1's ReLU, the max over
 * the template points and the ReLU after it run in fp32 (h1 is split again before layer 2), the store is fp32. There is no
 * sim_out. W1s / W2s: ptt_pack_weight_split_bf16 of the two (256,256) weights with the scale folded in. shift1 / shift2 may be
 * NULL (no shift). B == 0 or Ns == 0: PTT_OK, nothing is launched. A NULL descriptor or a NULL pointer among cos_t, P, w_sim,
 * W1s, W2s, out: PTT_EINVAL; P, w_sim, W1s or W2s not 16-byte aligned, or a negative output stride: PTT_EINVAL; Nt <= 0 or
 * Nt % 64 != 0: PTT_EUNSUPPORTED; an array of the launch over 2 GiB (32-bit offsets): PTT_EUNSUPPORTED. A refused call writes
 * nothing. */
typedef struct ptt_xcorr_split_desc {
    const float* cos_t;          /* (B,Ns,Nt) from ptt_cosine_map_f32 */
    const float* P;              /* (B,Nt,256) contiguous: layer 0's per-template-point term, BatchNorm folded in */
    const float* w_sim;          /* (256): layer 0's similarity column, scale folded */
    const void* W1s;             /* split pack, Cout = 256, K = 256 */
    const float* shift1;         /* (256) or NULL */
    const void* W2s;             /* split pack, Cout = 256, K = 256 */
    const float* shift2;         /* (256) or NULL */
    int relu2;                   /* layer 2's ReLU (after the max, which commutes with it) */
    float* out;                  /* element (b, c, j) at out[b*out_sb + c*out_sc + j*out_sn] */
    long long out_sb, out_sc, out_sn;
    int B, Ns, Nt;
} ptt_xcorr_split_desc;

int ptt_xcorr_split_f32(const ptt_xcorr_split_desc* d, ptt_stream_t stream);
/* order (B,N) i32: the points of every cloud along a Morton curve through the cloud's bounding box (flat indices b*N + n,
 * ties by index: a permutation inside each cloud), N <= 8192. Neighbours in space become neighbours in launch order. */
int ptt_spatial_order_f32(const float* xyz, int B, int N, int32_t* order, ptt_stream_t stream);

/* ---------------------------------------------------------------------------------
 * N4  device-side pre/post-processing of the sequential tracking loop
 * (tools/eval_utils/eval_tracking_utils.py:140-229,266-274). A tracklet's clouds stay resident in HBM; per frame
 * the host supplies the float64 box quantities of the previous result (a few dozen numbers) and receives one
 * (x, y, z, theta, score) row.
 *
 * ptt_crop_compact_f32 — one job = crop_center_pc (ptt/datasets/kitti/kitti_tracking_utils.py:300-339):
 *   keep points with lo1 < p < hi1 (crop_pc :281-298 in the cloud's frame; float32 point vs float64 bound, strict);
 *   p <- float32(p + trans) per axis (PointCloud.translate :44-46); p <- float32(rot . p) (PointCloud.rotate :48-49,
 *   float64 dot product); keep points with lo2 < p < hi2 (the second crop_pc, in the box frame). Survivors are
 *   written to `out` as (count, 3) float32 rows IN THEIR ORIGINAL ORDER; *count receives their number (rows beyond
 *   `capacity` are counted, not written). The job array lives in DEVICE memory (the caller uploads it).
 *   label_out != NULL (the training crop, crop_center_pc with gt_box, :308-312,322): label_out[r] = 1 where survivor r lies inside
 *   the ground-truth box — get_label_by_box (:238-272) evaluated on the first crop's points in the CLOUD's frame, i.e.
 *   p' = float32(lrot . float32(p + ltrans)), llo < p' < lhi with the ground-truth box's own translation / rotation / bounds —
 *   carried through the second crop exactly as crop_pc carries `label` (:295-296).
 *   append != 0 (SHAPE_AGGREGATION = all, whose template is get_model over every earlier frame, eval_tracking_utils.py:211-216):
 *   `out` already holds the crops of earlier launches and *count their running total; this crop's survivors are written after
 *   them (rows from `capacity` on are counted, not written) and *count is raised by their number. The total stays on the
 *   device, so a replayed job table needs no host-side offset; running the same job twice appends twice.
 * ------------------------------------------------------------------------------- */
typedef struct ptt_crop_job {
    const float* points;        /* (3, n_points) float32: row 0 = x, row 1 = y, row 2 = z (PointCloud.points) */
    int64_t ld;                 /* elements between rows */
    double lo1[3], hi1[3];
    double trans[3];
    double rot[9];              /* row-major 3x3 */
    double lo2[3], hi2[3];
    float* out;                 /* (capacity, 3) */
    int32_t* count;
    int32_t n_points;
    int32_t capacity;
    uint8_t* label_out;         /* (capacity) or NULL: the survivors' labels against the ground-truth box ... */
    double ltrans[3];           /* ... whose frame is p' = lrot . (p + ltrans), bounds llo < p' < lhi */
    double lrot[9];
    double llo[3], lhi[3];
    int32_t append;             /* 0: survivors from row 0, *count = their number; nonzero: appended to a running store (above) */
    int32_t reserved;           /* 0 */
} ptt_crop_job;

int ptt_crop_compact_f32(const ptt_crop_job* jobs_device, int n_jobs, ptt_stream_t stream);
/* The same crops with the job table in HOST memory, passed by value in the kernel arguments (n_jobs <=
 * PTT_CROP_JOBS_BY_VALUE_MAX): one tracklet's frame is two crops, and a per-frame host-to-device copy of the table in front
 * of the launch costs more than the launch. The table is read before the call returns. */
#define PTT_CROP_JOBS_BY_VALUE_MAX 8
int ptt_crop_compact_host_f32(const ptt_crop_job* jobs_host, int n_jobs, ptt_stream_t stream);

/* ptt_crop_scan_f32 (ABI 30) — the crops of ptt_crop_compact_f32 for clouds that are whole LiDAR scans (35k - 130k points, a few targets):
 * every job is spread over the chip instead of walking its cloud on one workgroup. Same job table (DEVICE memory), same
 * results bit for bit: the same survivors in their original order with the same float32 values (one shared per-point
 * function), *count = their number even where it exceeds `capacity`, rows from `capacity` on not written.
 *   Geometry: grid = (chunks of PTT_SCAN_CROP_CHUNK points of the longest cloud) x (jobs); a workgroup handles one chunk of one
 *   job. Two launches: the first writes the survivor count of every (job, chunk) into the workspace, the second adds up the
 *   counts of the chunks in front of it, repeats the test and writes its rows. No workgroup waits for another, nothing is
 *   placed by an atomic: the result does not depend on scheduling, and a second call writes identical bytes.
 *   max_points: the host's upper bound on every job's n_points; it sizes the grid. Chunks past a job's own n_points contribute
 *   nothing; a job with n_points = 0 gives *count = 0. Points from max_points (rounded up to a whole chunk) on are NOT looked at:
 *   the caller guarantees n_points <= max_points (the device cannot report a violation; ops.crop_scan checks the host table).
 *   ws / ws_bytes: ptt_crop_scan_workspace(n_jobs, max_points) bytes of device memory (one int32 per job and chunk), 4-byte
 *   aligned, overwritten by every call; less than that is PTT_EINVAL. n_jobs <= 65535.
 *   Not supported: label_out != NULL and append != 0 — both fields are IGNORED here (no labels are written, rows start at 0).
 *   Callers that hold the host table refuse such jobs before uploading (ops.crop_scan raises ValueError). */
#define PTT_SCAN_CROP_CHUNK 1024
size_t ptt_crop_scan_workspace(int n_jobs, int max_points);
int ptt_crop_scan_f32(const ptt_crop_job* jobs_device, int n_jobs, int max_points, void* ws, size_t ws_bytes, ptt_stream_t stream);

/* ptt_scan_ingest_f32 (ABI 34) — the sensor's raw rows into planar clouds in the reference frame: what
 * KittiTrackingDataset.get_lidar (ptt/datasets/kitti/kitti_dataset_tracking.py:298-308) does on the host with
 * np.fromfile(...).reshape(-1, 4).T, PointCloud.__init__ (kitti_tracking_utils.py:10-13: the first three rows) and
 * PointCloud.transform, and the nuScenes loader with rotate / translate / rotate / translate (nus_dataset_tracking.py:140-145).
 *   Per point: p = raw[i * row_floats + 0..2]; the steps are applied in order. A step is computed in float64 from the float32 p,
 *   every multiplication and addition rounded on its own (no fused multiply-add), and its result is rounded to float32 before
 *   the next step — the reference stores every step back into its float32 array:
 *     PTT_SCAN_ROTATE     p_r = float32((m[3r] * x + m[3r+1] * y) + m[3r+2] * z)                  m[0..8]  row-major 3x3
 *     PTT_SCAN_TRANSLATE  p_r = float32(p_r + m[r])                                               m[0..2]
 *     PTT_SCAN_AFFINE     p_r = float32(((m[4r] * x + m[4r+1] * y) + m[4r+2] * z) + m[4r+3])      m[0..11] row-major 3x4
 *   n_steps = 0 is a pure de-interleave, bit-exact. A `kind` that is none of the three is applied as the identity, n_steps is
 *   clamped to 0..PTT_SCAN_MAX_STEPS: the device cannot report what is inside the table, callers that hold the host table check
 *   it before the launch (ops.scan_ingest_check raises ValueError).
 *   The crop's own rotate (ptt_crop_compact_f32) forms the same sum with fused multiply-adds and is therefore NOT this function:
 *   the two agree except where the un-fused float64 sum lies within one float64 ulp of a float32 rounding boundary.
 *   Geometry: grid = (chunks of PTT_SCAN_CROP_CHUNK points of the longest job) x (jobs), one point per thread. max_points: the
 *   host's upper bound on every job's n_points; points from max_points (rounded up to a whole chunk) on are not looked at.
 *   Reads and writes: a job with n_points = 0 writes nothing; nothing outside out[r * ld + 0 .. n_points), r = 0..2, is written;
 *   `raw` is read one float at a time unless row_floats == 4 and `raw` is 16-byte aligned (then one 16-byte load per point).
 *   `jobs` may live in device memory or in PINNED host memory, as the crop table of ptt_crop_regularize_f32. One launch, no
 *   workspace, no atomics, no host synchronisation; it can be captured in a graph.
 *   PTT_EINVAL, before any runtime call: jobs == NULL, n_jobs outside 1..65535, max_points < 1 (or beyond 2^31 - 1 - chunk). */
#define PTT_SCAN_MAX_STEPS 4
#define PTT_SCAN_ROTATE    1
#define PTT_SCAN_TRANSLATE 2
#define PTT_SCAN_AFFINE    3
typedef struct ptt_scan_step {
    int32_t kind;               /* PTT_SCAN_ROTATE / _TRANSLATE / _AFFINE */
    int32_t reserved;           /* 0 */
    double m[12];
} ptt_scan_step;
typedef struct ptt_scan_job {
    const float* raw;           /* (n_points, row_floats) float32, 4-byte aligned */
    float* out;                 /* (3, n_points) planar, rows `ld` elements apart */
    int64_t ld;
    int32_t n_points;
    int32_t row_floats;         /* 3..16; columns from 3 on (intensity, ring, time) are dropped */
    int32_t n_steps;            /* 0..PTT_SCAN_MAX_STEPS */
    int32_t reserved;           /* 0 */
    ptt_scan_step steps[PTT_SCAN_MAX_STEPS];
} ptt_scan_job;
int ptt_scan_ingest_f32(const ptt_scan_job* jobs, int n_jobs, int max_points, ptt_stream_t stream);

/* ptt_scan_preload_f32 (ABI 34) — crop_pc (kitti_tracking_utils.py:275-297) without a change of frame, planar in and planar
 * out: the preload crop of get_lidar (kitti_dataset_tracking.py:309-310). Keeps the points with lo < p < hi on every axis (float32
 * point against float64 bound, strict, :281-292); the host forms lo / hi from the box's corners -/+ offset (:276-279).
 *   Survivors are written to `out` in their original order with their values unchanged; *count = their number, even above
 *   `capacity`; columns from `capacity` on are not written; out == NULL only counts.
 *   Two launches over grid = (chunks of PTT_SCAN_CROP_CHUNK points) x (jobs), exactly as ptt_crop_scan_f32 makes them: the first
 *   writes the survivor count of every (job, chunk) into the workspace, the second adds up the counts of the chunks in front,
 *   repeats the test and writes. No workgroup waits for another, nothing is placed by an atomic, a second call writes identical
 *   bytes. The job table lives in DEVICE memory. max_points as for ptt_crop_scan_f32.
 *   ws / ws_bytes: ptt_scan_preload_workspace(n_jobs, max_points) bytes of device memory, 4-byte aligned, overwritten by every call.
 *   PTT_EINVAL, before any launch: a short or misaligned workspace, a null pointer, n_jobs outside 1..65535, max_points < 1. */
typedef struct ptt_preload_job {
    const float* points;        /* (3, n_points) planar float32, rows `ld` elements apart */
    int64_t ld;
    int32_t n_points;
    int32_t capacity;
    double lo[3], hi[3];
    float* out;                 /* (3, capacity) planar, rows `out_ld` elements apart; NULL: count only */
    int64_t out_ld;
    int32_t* count;
} ptt_preload_job;
size_t ptt_scan_preload_workspace(int n_jobs, int max_points);
int ptt_scan_preload_f32(const ptt_preload_job* jobs_device, int n_jobs, int max_points, void* ws, size_t ws_bytes, ptt_stream_t stream);

/* ptt_regularize_f32 — one job = regularize_pc(pc, input_size, istrain=False) (kitti_tracking_utils.py:342-367) on the
 * concatenation of up to PTT_MAX_SEGMENTS compacted crops (get_model :219-236 concatenates the crops of several
 * frames): n = total rows; n <= 2 -> all-zero cloud; n == input_size -> copied through; otherwise row i of `out` is
 * point idx[i], idx = np.random.randint(0, n, input_size) drawn right after set_manual_seed(1), i.e. the 32-bit
 * outputs of MT19937(seed 1) masked to the smallest 2^k - 1 >= n - 1 and skipped while > n - 1. `draws` (DEVICE) holds
 * the generator's first n_draws outputs: fill a host buffer with ptt_mt19937_fill(1, ...) and upload it once;
 * n_draws >= 4 * input_size + 1024 always suffices (acceptance probability > 1/2). info (2 x int32, may be NULL)
 * receives n and the number of generator outputs consumed (0 when nothing was drawn). A draw table that runs out before
 * input_size indices were accepted leaves the rows in front valid (those the table did yield), every row from the
 * shortfall on NaN, and info[1] = -1. */
#define PTT_MAX_SEGMENTS 4
typedef struct ptt_regularize_job {
    const float* seg[PTT_MAX_SEGMENTS];          /* (seg_count, 3) float32 each */
    const int32_t* seg_count[PTT_MAX_SEGMENTS];  /* device scalars written by ptt_crop_compact_f32 */
    int32_t seg_capacity[PTT_MAX_SEGMENTS];
    float* out;                                  /* (input_size, 3) */
    int32_t* info;
    int32_t n_seg;
    int32_t input_size;
} ptt_regularize_job;

int ptt_regularize_f32(const ptt_regularize_job* jobs_device, int n_jobs, const uint32_t* draws, int n_draws,
                       ptt_stream_t stream);
/* ptt_crop_compact_f32 + ptt_regularize_f32 of one frame in ONE launch: workgroup w runs crop job w and then resampling job w
 * (whose segments are that crop's output and, for a template, crops of earlier launches) — identical results. crop_jobs may
 * live in device memory or in PINNED host memory (read through unified addressing: the launch can sit in a hipGraph whose
 * table the host rewrites between replays); reg_jobs_device as for ptt_regularize_f32. */
int ptt_crop_regularize_f32(const ptt_crop_job* crop_jobs, const ptt_regularize_job* reg_jobs_device, int n_jobs,
                            const uint32_t* draws, int n_draws, ptt_stream_t stream);

/* First n outputs of MT19937 seeded with init_genrand(seed) (what np.random.seed(seed) followed by 32-bit draws
 * yields) into a HOST buffer — the one entry point that takes a host pointer. */
int ptt_mt19937_fill(uint32_t seed, uint32_t* out_host, int n);

/* Host-side float64 box arithmetic of the tracking loop (HOST pointers, no device work): what the reference does per
 * frame through `Box` / pyquaternion (kitti_tracking_utils.py:68-160,186-216,300-339), batched over n tracklets so
 * that a step of 48 interleaved tracklets costs microseconds of host time. Quaternions are (w, x, y, z).
 *
 * ptt_track_crop_bounds — the float64 quantities of crop_center_pc(pc, box, offset=offset, scale=scale) per box
 *   (lo1/hi1: crop_pc with 2*offset, 4*scale in the cloud's frame; trans = -center; rot = R^T; lo2/hi2: crop_pc of the
 *   carried-along box with offset + extra2[i] (extra2 NULL = 0; gt_box.wlh[1]*0.6 for the search crop, :321) and scale)
 *   written into jobs_host[i * job_stride] (the other fields are left untouched).
 * ptt_track_box_by_offset — boxes[i] <- get_box_by_offset(boxes[i], offsets[i*offset_stride .. +4), use_z) for every i
 *   with active[i] != 0 (active NULL = all). offsets are the model's float32 outputs (x, y, z, theta in degrees); the
 *   angle is formed as the float32 product the reference forms. An x / y offset larger than the box is redrawn from
 *   U(-1, 1) (:205-208) using the two next 32-bit outputs of MT19937(seed 1) at position rng_pos[i] (the state numpy's
 *   global generator has after regularize_pc's resampling consumed rng_pos[i] outputs); rng_pos[i] advances by 2 per
 *   draw; offsets are updated in place with the values used. */
typedef struct ptt_track_box {
    double center[3];
    double wlh[3];
    double quat[4];
} ptt_track_box;

int ptt_track_crop_bounds(const ptt_track_box* boxes, int n, double offset, double scale, const double* extra2,
                          ptt_crop_job* jobs_host, int job_stride);
int ptt_track_box_by_offset(ptt_track_box* boxes, int n, float* offsets, int offset_stride, int use_z,
                            const int32_t* active, int64_t* rng_pos);
/* The host side of post_process for one step in one call: per tracklet the first arg-max of the scores out of the (n,P,5) read-back
 * (P == 1: rows already selected) -> est_out (n,5); rng_pos[i] <- the draw count of this frame's resampling (info (n,2,2) int32 =
 * (points, draws used) of search / template: the template's if it resampled, else the search's; a negative count = the draw table
 * ran out: PTT_EINVAL); then ptt_track_box_by_offset(boxes, est_out, ...). */
int ptt_track_select_update(const float* proposals_host, int P, const int32_t* info_host, ptt_track_box* boxes, int n, int use_z,
                            const int32_t* active, int64_t* rng_pos, float* est_out);

/* ptt_select_box_f32 — post_process (eval_tracking_utils.py:266-274): for every frame b the row of
 * pred_box_data (B,P,5) with the largest score (column 4; first one among equals, as np.argmax) -> out (B,5);
 * idx_out (B) receives its index, or NULL. A NaN score counts as the maximum, again as np.argmax: the first NaN of a row wins,
 * which is also what ptt_track_select_update chooses on the host. Every score -inf: row 0. */
int ptt_select_box_f32(const float* pred_box_data, int B, int P, float* out, int32_t* idx_out, ptt_stream_t stream);

/* ptt_box_overlap_f64 (ABI 27) — the two numbers the reference scores a tracked frame by (tools/eval_utils/
 * eval_tracking_metrics.py:37-74), for n (ground truth, result) box pairs in one launch, one pair per thread, all in float64:
 *   overlap[i]  = estimateOverlap(gt[i], pred[i], dims, ref_coord)     accuracy[i] = estimateAccuracy(gt[i], pred[i], dims)
 * gt / pred: n boxes in the ptt_track_box layout (centre 3, wlh 3, quaternion w x y z), DEVICE memory.
 *   equality   overlap = 1.0 exactly when every one of the 10 numbers has |gt - pred| <= 1e-8 + 1e-5 * |pred|: Box.__eq__
 *              (kitti_tracking_utils.py:84-93), i.e. np.allclose(gt, pred), asymmetric as numpy's is;
 *   footprint  four of Box.corners (:132-150; the quaternion is general, not only a yaw): PTT_REF_CAMERA corners 0, 1, 5, 4 on
 *              (x, z), PTT_REF_LIDAR corners 2, 3, 7, 6 (bottom_corners) on (x, y); each quadrilateral is put in
 *              counter-clockwise order by its signed area, gt's is clipped by the four half-planes of pred's (Sutherland-Hodgman,
 *              at most 8 vertices), the area is the shoelace sum, fewer than 3 vertices = 0;
 *   dims == 2  inter / (area_gt + area_pred - inter), the areas those of the two footprints;
 *   dims == 3  inter * max(0, ymax - ymin) / (vol_gt + vol_pred - that), vol = w * l * h, ymax = min(centre_y), ymin =
 *              max(centre_y - h) — formed from component 1 of the centres under BOTH conventions, as the reference does (:65-67);
 *   accuracy   |centre_gt - centre_pred|, dims == 2: over components 0 and 2 (:41-42).
 * Boxes with a non-positive size are outside the contract. Another dims or ref_coord: PTT_EINVAL; n == 0 launches nothing. */
#define PTT_REF_CAMERA 0
#define PTT_REF_LIDAR 1
int ptt_box_overlap_f64(const double* gt, const double* pred, int n, int ref_coord, int dims, double* overlap, double* accuracy,
                        ptt_stream_t stream);

/* ---------------------------------------------------------------------------------
 * N5 (ABI 28)  device-resident training batches: the reference's get_train_items (ptt/datasets/kitti/
 * kitti_dataset_tracking.py:60-179), batched. A batch of B samples is drawn from B + spare CANDIDATES (B primaries, then the
 * spares that stand in for rejected primaries) in two launches, with no count ever crossing PCIe:
 *   launch 1  ptt_crop_compact_f32 over 3 jobs per candidate: the search crop with labels (prepare_search_and_label :120-138),
 *             the first-frame and the previous-frame template crop (get_model, prepare_template_data :151-174) into per-candidate
 *             scratch sized for the largest resident cloud; the three counts stay on the device;
 *   launch 2  ptt_train_batch_f32, one workgroup per output slot b < B:
 *     validity    candidate c is valid when n_search > min_points and n_first + n_prev > min_points (:140, :176: a crop of
 *                 <= 20 points rejects the sample);
 *     source      a valid primary b is its own source. An invalid one takes the r-th valid spare, r = the number of invalid
 *                 primaries before b (the reference retries a uniformly random index, :76,:99: the spares are such indices, drawn
 *                 by the host). With fewer valid spares than that (a SHORTFALL) it takes valid candidate number
 *                 (r - n_valid_spares) mod n_valid, counted over primaries then spares; with no valid candidate at all the slot is
 *                 all zeros and its source -1;
 *     resampling  regularize_pc(istrain=True) (kitti_tracking_utils.py:342-367): n == size -> the rows in order; otherwise row i
 *                 of the output is row idx_i of the crop, idx_i = (uint64(w_i) * n) >> 32 with w_i = word i & 3 of
 *                 Philox4x32-10(counter = (i >> 2, index, which, epoch), key = (seed_lo, seed_hi)), which = 0 search, 1 template
 *                 (Salmon et al., SC'11; bias n / 2^32, no rejection, no generator state: the reference's np.random.randint draws
 *                 from numpy's per-worker global generator, which no device can follow). The search labels ride on the same
 *                 indices (:354-355) and come out as float32 0 / 1; the template is resampled over first || previous;
 *     reg_label   the candidate's four float32 values (formed in float64 by the host, :324); src_out[b] = the source candidate;
 *     idx_*_out   (may be NULL) the drawn indices, -1 throughout for a pass-through or an all-zero slot;
 *     info        (may be NULL) 4 x int32 written by slot 0's workgroup: invalid primaries, valid spares, shortfall =
 *                 max(0, invalid primaries - valid spares), all_invalid (0 / 1); totals (may be NULL) 4 x int64 raised by the same
 *                 thread: batches, then the running sums of the first three of those. Batches that share `totals` must run on one stream.
 * The candidate table lives in DEVICE memory; the descriptor is HOST memory, read before the call returns (passed by value with
 * the launch). The outputs need only their element alignment: rows are written as float4 / int4 where the size is a multiple
 * of four and the base pointers are 16-byte aligned, element by element otherwise. Every address is fixed by the tables, so both launches replay from a hipGraph. 1 <= B <= n_cand <=
 * PTT_TRAIN_MAX_CANDS, sizes >= 1, min_points >= 2; anything else: PTT_EINVAL.
 * ------------------------------------------------------------------------------- */
#define PTT_TRAIN_MAX_CANDS 1024
typedef struct ptt_train_cand {
    const float* search;        /* (capacity, 3) the search crop, (capacity) its labels: a label job's out / label_out */
    const uint8_t* label;
    const float* first;         /* (capacity, 3) the template's two crops */
    const float* prev;
    const int32_t* counts;      /* 3 device scalars: rows of search, first, prev (the crop jobs' counts; clamped to capacity) */
    float reg[4];               /* reg_label */
    uint32_t index;             /* the dataset index: word 1 of the Philox counter */
    uint32_t epoch;             /* word 3 */
    int32_t capacity;
    int32_t reserved;           /* 0 */
} ptt_train_cand;

typedef struct ptt_train_batch_desc {
    float* search_points;       /* (B, search_size, 3) */
    float* template_points;     /* (B, template_size, 3) */
    float* cls_label;           /* (B, search_size) */
    float* reg_label;           /* (B, 4) */
    int32_t* src_out;           /* (B) */
    int32_t* idx_search_out;    /* (B, search_size) or NULL */
    int32_t* idx_template_out;  /* (B, template_size) or NULL */
    int32_t* info;              /* (4) or NULL */
    int64_t* totals;            /* (4) or NULL */
    int32_t B, n_cand;
    int32_t search_size, template_size;
    int32_t min_points;
    uint32_t seed_lo, seed_hi;  /* the Philox key */
    int32_t reserved;           /* 0 */
} ptt_train_batch_desc;

int ptt_train_batch_f32(const ptt_train_cand* cands_device, const ptt_train_batch_desc* desc_host, ptt_stream_t stream);

/* (ABI 35) The same batch with the sample's DATA_AUGMENTOR applied (ptt/datasets/augmentor: random_world_flip, _rotation and
 * _scaling in any order compose to one map). aug_device: n_cand records in DEVICE memory, parallel to the candidate table. The
 * workgroup of slot b reads the record of its SOURCE candidate and stores, for every row (x, y, z) of search_points and
 * template_points,  x' = m[0] x + m[1] y,  y' = m[2] x + m[3] y,  z' = kz z  in float32. Labels, indices, src_out, info and
 * totals are as without it; reg_label arrives augmented from the host, as it arrives at all; a slot without a source stays all
 * zeros. aug_device == NULL is ptt_train_batch_f32 (which forwards here). Same argument checks. */
typedef struct ptt_train_aug {
    float m[4];                 /* m00, m01, m10, m11 */
    float kz;
    float reserved[3];          /* 0 */
} ptt_train_aug;

int ptt_train_batch_aug_f32(const ptt_train_cand* cands_device, const ptt_train_aug* aug_device, const ptt_train_batch_desc* desc_host,
                            ptt_stream_t stream);
/* The generator of the resampling on the host (HOST pointers, no device work), for tests and tools: out4[0..3] =
 * Philox4x32-10(counter4, key2). */
int ptt_philox4x32_10(const uint32_t* counter4, const uint32_t* key2, uint32_t* out4);

/* ---------------------------------------------------------------------------------
 * N3  training step of the shared-MLP stages on hand-written kernels. The reference's SharedMLP in train mode is
 * [1x1 conv (no bias) -> BatchNorm with batch statistics -> ReLU] x 3 followed by a max over the neighbour axis
 * (pytorch_utils.py:12-36,94-114; pointnet2_modules.py:84-88; similarity_modules/p2b_xcoor.py:39-41), and
 * loss.backward() (tools/train_utils/train_utils.py:47-48) runs their backward. Activations are (R, C) ROWS (one row
 * per (centre, neighbour) position, channels contiguous): the convolution and its input gradient are ptt_linear_f32,
 * the rest is below. Every reduction runs in a fixed order (float64 partials per 2048 / 4096-row chunk, combined in
 * chunk order): bit-reproducible.
 *
 * ptt_bn_stats_f32      per-channel batch statistics of X (R,C): mean, BIASED variance, invstd = 1/sqrt(var + eps)
 *                       (BatchNorm2d forward in train mode; the caller updates running_mean / running_var).
 * ptt_bn_apply_f32      X = relu?((Z - mean) * invstd * gamma + beta)
 * ptt_bn_bwd_f32        backward of BatchNorm(train) + ReLU: dy = G where Act > 0 else 0; dbeta = sum dy;
 *                       dgamma = sum dy * xhat; dZ = gamma * invstd * (dy - dbeta / R - xhat * dgamma / R).
 * ptt_pool_rows_f32     out[g,c] = max_k X[g*ns + k, c], arg = first arg-max   (F.max_pool2d over the neighbour axis)
 * ptt_pool_rows_bwd_f32 dX[g*ns + k, c] = dOut[g,c] if k == arg[g,c] else 0
 * ptt_linear_wgrad_f32  dW[o,i] (+)= sum_r dZ[r,o] * X[r,i] on fp32 MFMA (the weight gradient of a 1x1 convolution /
 *                       nn.Linear over R rows), split over 4096-row chunks.
 * ------------------------------------------------------------------------------- */
size_t ptt_bn_stats_workspace(int R, int C);
int ptt_bn_stats_f32(const float* X, int R, int C, int ldx, float eps, float* mean, float* var, float* invstd,
                     void* workspace, size_t workspace_bytes, ptt_stream_t stream);
int ptt_bn_apply_f32(const float* Z, int ldz, const float* mean, const float* invstd, const float* gamma,
                     const float* beta, int R, int C, int relu, float* X, int ldx, ptt_stream_t stream);
int ptt_bn_bwd_f32(const float* G, int ldg, const float* Act, int lda, const float* Z, int ldz, const float* mean,
                   const float* invstd, const float* gamma, int R, int C, int relu, float* dZ, int ldd,
                   float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, const float* act_scale,
                   const float* act_shift, ptt_stream_t stream);
/* SyncBatchNorm (tools/train_tracking.py:133-134, --sync_bn -> nn.SyncBatchNorm.convert_sync_batchnorm): the same
 * statistics split where the ranks exchange them. Forward: ptt_bn_sums_f64 -> all-reduce(sums, row count) ->
 * ptt_bn_finish_f64. Backward: ptt_bn_bwd_sums_f64 (sum dy, sum dy * xhat; a rank's dbeta / dgamma are its LOCAL sums,
 * as torch's SyncBatchNorm keeps them) -> all-reduce -> ptt_bn_bwd_apply_f32 with the global sums and the global count.
 * Forward sums = 2 * C + 1 doubles: sum, sum of squares, and in the last slot the row count R — so one all-reduce carries
 * everything and the global count never visits the host; ptt_bn_finish_f64 and ptt_bn_bwd_apply_f32 (count = a device
 * pointer to that slot) read it from device memory. Backward sums = 2 * C doubles. Fixed combination order; C % 4 == 0,
 * 16-byte aligned rows. */
int ptt_bn_sums_f64(const float* X, int R, int C, int ldx, double* sums, void* workspace, size_t workspace_bytes,
                    ptt_stream_t stream);
int ptt_bn_finish_f64(const double* sums, int C, float eps, float* mean, float* var, float* invstd,
                      ptt_stream_t stream);
int ptt_bn_bwd_sums_f64(const float* G, int ldg, const float* Act, int lda, const float* Z, int ldz, const float* mean,
                        const float* invstd, int R, int C, double* sums, void* workspace, size_t workspace_bytes,
                        const float* act_scale, const float* act_shift, ptt_stream_t stream);
int ptt_bn_bwd_apply_f32(const float* G, int ldg, const float* Act, int lda, const float* Z, int ldz, const float* mean,
                         const float* invstd, const float* gamma, const float* sum_dy, const float* sum_dy_xhat,
                         const double* count, int R, int C, float* dZ, int ldd, const float* act_scale, const float* act_shift,
                         ptt_stream_t stream);
int ptt_pool_rows_f32(const float* X, int ldx, int G, int ns, int C, float* out, int ldo, int32_t* arg,
                      const float* act_scale, const float* act_shift, ptt_stream_t stream);
int ptt_pool_rows_bwd_f32(const float* dOut, int ldo, const int32_t* arg, int G, int ns, int C, float* dX, int ldx,
                          ptt_stream_t stream);
/* Point-Transformer block in training mode (transformer_block/variants.py:156-163): the element-wise chains around its
 * GEMMs over the (B,N,k,D) per-(point, neighbour) tensors, one pass each (k = 16, D % 4 == 0; q / kf / vf are (B,N,D)
 * point rows, knn (B,N,k) int32, pos / a / t / attn / da / dvp (B,N,k,D)):
 *   ptt_pt_pair_input_f32      t = q_i - kf[knn_ij] + pos_ij                                  (argument of fc_gamma, :160)
 *   ptt_pt_attn_train_fwd_f32  attn = softmax_j(a * scale); res_i = sum_j attn_ij * (vf[knn_ij] + pos_ij)      (:161-163)
 *   ptt_pt_attn_train_bwd_f32  from dres: dvp_ij = attn_ij * dres_i (gradient of v[knn] and of pos),
 *                              da_ij = attn_ij * (dres_i.vp_ij - sum_j' attn_ij' dres_i.vp_ij') * scale          */
int ptt_pt_pair_input_f32(const float* q, const float* kf, const int32_t* knn, const float* pos, int B, int N, int k, int D,
                          float* t, ptt_stream_t stream);
int ptt_pt_attn_train_fwd_f32(const float* a, const float* vf, const int32_t* knn, const float* pos, int B, int N, int k, int D,
                              float scale, float* attn, float* res, ptt_stream_t stream);
int ptt_pt_attn_train_bwd_f32(const float* attn, const float* vf, const int32_t* knn, const float* pos, const float* dres, int B,
                              int N, int k, int D, float scale, float* da, float* dvp, ptt_stream_t stream);

/* The same two passes with row strides for q / k / v (column slices of the stacked (B,N,3D) projection) and an optional attention
 * output (attn may be NULL): the per-layer INFERENCE form of the block for a handful of frames, where the fused pair kernel's
 * one workgroup per two points leaves most CUs idle (one tracklet frame: 64 workgroups) — ptt_amd/models/transformer_block. */
int ptt_pt_pair_input_ld_f32(const float* q, int ldq, const float* kf, int ldk, const int32_t* knn, const float* pos, int B, int N,
                             int k, int D, float* t, ptt_stream_t stream);
int ptt_pt_attn_fwd_ld_f32(const float* a, const float* vf, int ldv, const int32_t* knn, const float* pos, int B, int N, int k, int D,
                           float scale, float* attn, float* res, ptt_stream_t stream);

/* Grouping of point-major rows and its deterministic backward (the training-mode layer-0 hoist: the first MLP layer's
 * feature half is evaluated once per point, then gathered per (centre, neighbour) row):
 *   ptt_gather_rows_f32       out[b,e,:] = src[b, idx[b,e], :]        src (B,N,C), idx (B,E) -> out (B,E,C); C % 4 == 0
 *   ptt_scatter_csr_i32       order (B,E) / start (B,N+1): the entries of every cloud sorted by (idx, e) — a stable counting sort
 *                             up to 2048 bins (any E), a bitonic network in LDS above (E <= 16384)
 *   ptt_scatter_rows_csr_f32  out[b,n,:] = sum of g[b,e,:] over idx[b,e] == n in ascending e (fixed order) */
int ptt_gather_rows_f32(const float* src, const int32_t* idx, int B, int N, int E, int C, float* out, ptt_stream_t stream);
int ptt_scatter_csr_i32(const int32_t* idx, int B, int N, int E, int32_t* order, int32_t* start, ptt_stream_t stream);
int ptt_scatter_rows_csr_f32(const float* g, const int32_t* order, const int32_t* start, int B, int N, int E, int C,
                             float* out, ptt_stream_t stream);
/* The last layer of a SharedMLP + max-pool stage in training (pytorch_utils.py:12-36 + F.max_pool2d, pointnet2_modules.py:84-88)
 * without the pooling pass over its (rows, N) output: ptt_rows_gemm_f32 with statistics whose epilogue ALSO takes, per group of
 * `ns` consecutive rows and per column, the largest and the smallest output with the first row (inside the group) holding it —
 * pmax / pmin (rows / ns, N) float, amax / amin (rows / ns, N) int32. Once the batch statistics (summed by the same launch) give
 * the BatchNorm's a = gamma * invstd and b = beta - mean * a, ptt_pool_select_f32 forms the pooled relu(a y + b) and its arg-max:
 * relu(a y + b) is monotone in y, the sign of a picks max or min. in_scale / in_shift (the producing layer's deferred activation)
 * are required; shapes: ptt_rows_gemm_pool_supported (K, N multiples of 128 with ns 16 / 32 / 64, or K % 64 == 0, N % 128 == 0 with ns 32). */
int ptt_rows_gemm_pool_supported(int rows, int K, int N, int ldx, int ns);
int ptt_rows_gemm_pool_f32(const float* X, int rows, int K, int ldx, const float* in_scale, const float* in_shift,
                           const float* Wpacked, int N, float* out, int ldo, double* stats, size_t stats_elems, int ns,
                           float* pmax, float* pmin, int32_t* amax, int32_t* amin, ptt_stream_t stream);
int ptt_pool_select_f32(const float* pmax, const float* pmin, const int32_t* amax, const int32_t* amin, const float* act_scale,
                        const float* act_shift, int G, int C, float* out, int32_t* arg, ptt_stream_t stream);
/* out[c] = sum over the R rows of X[r][c] — the bias gradient of a row-wise layer (nn.Linear / Conv1d(k=1) backward,
 * transformer_block/variants.py:154-164 in training) — in a fixed order: bit-reproducible. Any C and ldx >= C: float4 loads where
 * C % 4 == 0, ldx % 4 == 0 and X and the partials' destination (the workspace; `out` itself when R fits one chunk) are 16-byte
 * aligned, scalar loads otherwise (the 259-channel vote layer, row views at an odd offset). */
size_t ptt_colsum_workspace(int R, int C);
int ptt_colsum_f32(const float* X, int R, int C, int ldx, float* out, void* workspace, size_t workspace_bytes, ptt_stream_t stream);
size_t ptt_linear_wgrad_workspace(int R, int Cout, int Cin);
int ptt_linear_wgrad_f32(const float* dZ, int ldz, const float* X, int ldx, int R, int Cout, int Cin, float* dW,
                         int accumulate, void* workspace, size_t workspace_bytes, const float* x_scale, const float* x_shift,
                         ptt_stream_t stream);
/* Deferred activation (training): a layer's output relu(z * a[c] + b[c]) (a = gamma * invstd, b = beta - mean * a) is
 * never written; its consumers apply it while they load z — ptt_linear_act_in_f32 (the next convolution),
 * ptt_linear_wgrad_f32's x_scale / x_shift (that convolution's weight gradient), ptt_pool_rows_f32's act_scale /
 * act_shift (the max-pool), ptt_bn_bwd_f32 with Act == NULL (the ReLU mask is z * a + b > 0). NULL scales = no transform. */
int ptt_linear_act_in_f32(const float* X, int rows, int K, int ldx, const float* in_scale, const float* in_shift,
                          const float* Wpacked, int Cout, float* out, int ldo, ptt_stream_t stream);

/* ---------------------------------------------------------------------------------
 * T-opt  the dense scaled-dot-product variant TransformerBlockSTD (transformer_block/variants.py:29-40): the only
 * literal Q.K^T / attn.V of the reference, as batched fp32-MFMA GEMMs.
 *   ptt_pack_weight_strided_f32  packs `batch` matrices given by strides into MFMA B-fragment order: element
 *                                (output o, input k) of batch b at W[b*stride_batch + o*stride_out + k*stride_k].
 *                                K of a batch (rows of the q|k|v buffer) -> the B operand of Q.K^T; V + delta read
 *                                transposed (stride_out 1, stride_k = row stride) -> the B operand of attn.V.
 *   ptt_linear_batched_f32       ptt_linear_f32 over `batch` independent (X, Wpacked, out[, residual]) sets.
 *   ptt_softmax_rows_f32         in-place softmax(scale * x) along the rows of a (rows, n) matrix (`attn / sqrt(d)`, :35).
 * ------------------------------------------------------------------------------- */
int ptt_pack_weight_strided_f32(const float* W, int Cout, int K, int64_t stride_out, int64_t stride_k, int batch,
                                int64_t stride_batch, float* packed, ptt_stream_t stream);
int ptt_linear_batched_f32(const float* X, int rows, int K, int ldx, int64_t x_batch_stride, const float* Wpacked,
                           int64_t w_batch_stride, int Cout, const float* scale, const float* shift, int relu,
                           const float* residual, int ldr, int64_t r_batch_stride, float* out, int ldo,
                           int64_t o_batch_stride, int batch, ptt_stream_t stream);
int ptt_softmax_rows_f32(float* X, int64_t rows, int n, int ld, float scale, ptt_stream_t stream);
/* out = LayerNorm_C(x) (+ residual): nn.LayerNorm(C) over the rows of a (rows, C) matrix (multitransformer.py:59-60 norm1,
 * norm2), one wave per row, fp32, mean then the variance of the centred values; weight / bias / residual may be NULL.
 * C <= 1024. out may alias x. */
int ptt_layernorm_f32(const float* x, int rows, int C, int ldx, const float* weight, const float* bias, float eps,
                      const float* residual, int ldr, float* out, int ldo, ptt_stream_t stream);

/* ---------------------------------------------------------------------------------
 * N3  the row GEMMs of the training step at 10^4 - 10^6 rows (round 3): a persistent, software-pipelined form of
 * ptt_linear_f32 / ptt_linear_wgrad_f32 for the forward, input-gradient and weight-gradient GEMMs of every 1x1
 * convolution and nn.Linear the training step runs over (centre, neighbour) / (point, neighbour) rows:
 *   SharedMLP convolutions and their backward      pytorch_utils.py:12-36 (loss.backward(): tools/train_utils/train_utils.py:47-48)
 *   TransformerBlock fc1, w_qs/w_ks/w_vs, fc_delta[2], fc_gamma[0], fc_gamma[2], fc2       transformer_block/variants.py:154-165
 *   the Conv1d stacks of the heads                 voting_heads/centroids_voting_head.py:15-21, box_voting_head.py:25
 * ptt_rows_gemm_f32:  out[r, :] = relu?( act_in(X[r, :]) . W^T + bias ) (+ residual[r, :]),  act_in(x) = relu(x * in_scale + in_shift)
 *   when in_scale / in_shift are given (the producing layer's BatchNorm + ReLU, never materialised), else x.
 *   Wpacked from ptt_pack_weight_f32 (Cout = N, K). Needs K % 64 == 0, N % 64 == 0, ldx % 4 == 0, 16-byte aligned X
 *   (ptt_rows_gemm_supported says so; otherwise use ptt_linear_f32).
 *   stats != NULL (then bias must be NULL): also the per-channel sums and sums of squares of `out` over the rows — the
 *   BatchNorm batch statistics of a convolution output without a second pass over it — as float64 partials
 *   stats[chunk][2][N], chunk < ptt_rows_gemm_stat_chunks(rows, K, N) (a pure function of the shape: the summation order
 *   is fixed); ptt_bn_finish_partials_f32 / ptt_bn_sums_partials_f64 combine them in chunk order.
 * ptt_linear_wgrad2_f32: ptt_linear_wgrad_f32 with up to 256 x 256 outputs per workgroup (every operand row read once);
 *   needs R >= 2048, Cout % 128 == 0, Cin % 128 == 0; same partial-sum scheme (fixed order), own workspace size. */
int ptt_rows_gemm_supported(int rows, int K, int N, int ldx, int ldo);
int ptt_rows_gemm_stat_chunks(int rows, int K, int N);
int ptt_rows_gemm_f32(const float* X, int rows, int K, int ldx, const float* in_scale, const float* in_shift,
                      const float* Wpacked, int N, const float* bias, int relu, const float* residual, int ldr,
                      float* out, int ldo, double* stats, size_t stats_elems, ptt_stream_t stream);
/* the input gradient of a Linear + ReLU layer's successor, masked by that ReLU: out = (mask > 0) ? X . W^T : 0, mask = the
 * ReLU's output (rows, N), row stride ldm; statistics (optional) are those of the MASKED output, whose column sums are
 * the bias gradient of the masked layer (nn.Sequential(Linear, ReLU, Linear): fc_delta / fc_gamma, variants.py:139-148). */
int ptt_rows_gemm_masked_f32(const float* X, int rows, int K, int ldx, const float* Wpacked, int N, const float* mask, int ldm,
                             float* out, int ldo, double* stats, size_t stats_elems, ptt_stream_t stream);
/* The input gradient g = dZ_next . W_next of a layer whose INPUT is relu(BatchNorm(Z)) (Z = the producing layer's convolution
 * output, deferred activation act_scale / act_shift): the GEMM's epilogue also takes that producing layer's BatchNorm backward
 * sums, sum dy and sum dy * xhat with dy = g where Z * act_scale + act_shift > 0, as float64 partials [chunk][2][N] — the pass
 * over (g, Z) that ptt_bn_bwd_f32 starts with disappears. ptt_bn_bwd_from_partials_f32 combines the partials (dbeta, dgamma) and
 * writes dZ; ptt_bn_bwd_sums_partials_f64 is the SyncBatchNorm form of the combine (all-reduce, then ptt_bn_bwd_apply_f32). */
int ptt_rows_gemm_bnbwd_f32(const float* X, int rows, int K, int ldx, const float* Wpacked, int N, const float* Z, int ldz,
                            const float* mean, const float* invstd, const float* act_scale, const float* act_shift, float* out,
                            int ldo, double* sums_partial, size_t partial_elems, ptt_stream_t stream);
int ptt_bn_bwd_from_partials_f32(const double* partial, int chunks, const float* G, int ldg, const float* Z, int ldz, const float* mean,
                                 const float* invstd, const float* gamma, int R, int C, float* dZ, int ldd, float* dgamma, float* dbeta,
                                 const float* act_scale, const float* act_shift, ptt_stream_t stream);
int ptt_bn_bwd_sums_partials_f64(const double* partial, int chunks, int C, double* sums, ptt_stream_t stream);
/* Round 5: the BatchNorm + ReLU backward of a layer APPLIED BY ITS CONSUMER. With dbeta = sum dy, dgamma = sum dy * xhat
 *   dz = gamma * invstd * (dy - dbeta / R - xhat * dgamma / R) = c0 + c1 * (z - mean) + (mask ? k1 * g : 0)
 * (k1 = gamma * invstd, c1 = -k1 * invstd * dgamma / R, c0 = -k1 * dbeta / R): three per-channel
 * constants instead of a pass that reads g and z and writes dz (ptt_bn_bwd_from_partials_f32 / ptt_bn_bwd_pooled_f32's last
 * launch, 1.5 ms of a 21-ms training step). ptt_bn_bwd_consts_f32 combines the partials of ptt_rows_gemm_bnbwd_f32 (dense
 * gradient), ptt_bn_bwd_pooled_consts_f32 sums over a POOLED gradient first (as ptt_bn_bwd_pooled_f32); both write dgamma,
 * dbeta and the constants. ptt_rows_gemm_bnbwd_fused_f32 = ptt_rows_gemm_bnbwd_f32 whose A operand is that dz, formed while
 * its rows are staged, and (dz_out) written out once for the layer's weight gradient. */
typedef struct ptt_bn_bwd_input {
    const float* g; int ldg;            /* dense: the gradient w.r.t. the layer's activated output (R,K); pooled: (R / ns, K) */
    const int32_t* arg; int ns;         /* pooled: arg-max row inside every group of ns rows, (R / ns, K) contiguous; NULL, 0: dense */
    const float* z; int ldz;            /* the layer's convolution output (R,K) */
    const float* k1; const float* c0; const float* c1; const float* mean;
    const float* act_a; const float* act_b;     /* the ReLU mask: z * act_a + act_b > 0 */
    float* dz_out; int ldd;             /* optional (R,K): dz written by the launch */
} ptt_bn_bwd_input;
int ptt_bn_bwd_consts_f32(const double* partial, int chunks, const float* mean, const float* invstd, const float* gamma, int R, int C,
                          float* dgamma, float* dbeta, float* k1, float* c0, float* c1, ptt_stream_t stream);
int ptt_bn_bwd_pooled_consts_f32(const float* dPooled, int ldp, const int32_t* arg, int ns, const float* Z, int ldz, const float* mean,
                                 const float* invstd, const float* gamma, int R, int C, float* dgamma, float* dbeta, float* k1,
                                 float* c0, float* c1, void* workspace, size_t workspace_bytes, const float* act_scale,
                                 const float* act_shift, ptt_stream_t stream);
int ptt_rows_gemm_bnbwd_fused_supported(int rows, int K, int N, int ns);
int ptt_rows_gemm_bnbwd_fused_f32(const ptt_bn_bwd_input* in, int rows, int K, const float* Wpacked, int N, const float* Z, int ldz,
                                  const float* mean, const float* invstd, const float* act_scale, const float* act_shift, float* out,
                                  int ldo, double* sums_partial, size_t partial_elems, ptt_stream_t stream);
int ptt_bn_finish_partials_f32(const double* partial, int chunks, int C, int R, float eps, float* mean, float* var, float* invstd,
                               ptt_stream_t stream);
int ptt_bn_sums_partials_f64(const double* partial, int chunks, int C, int R, double* sums, ptt_stream_t stream);
/* BatchNorm(train) + ReLU backward of the LAST layer of a SharedMLP + max-pool stage, with the gradient still POOLED:
 * dy[g*ns + k, c] = dPooled[g, c] if k == arg[g, c] else 0 (F.max_pool2d's backward, pointnet2_modules.py:84-88) is formed
 * on the fly — ptt_pool_rows_bwd_f32's (R, C) tensor is never written, the two sums run over G x C entries instead of R x C.
 * The ReLU mask is z * act_scale + act_shift > 0 (deferred activation). _sums / _apply: the SyncBatchNorm split, as
 * ptt_bn_bwd_sums_f64 / ptt_bn_bwd_apply_f32. Workspace: ptt_bn_stats_workspace(R, C). */
int ptt_bn_bwd_pooled_f32(const float* dPooled, int ldp, const int32_t* arg, int ns, const float* Z, int ldz, const float* mean,
                          const float* invstd, const float* gamma, int R, int C, float* dZ, int ldd, float* dgamma, float* dbeta,
                          void* workspace, size_t workspace_bytes, const float* act_scale, const float* act_shift, ptt_stream_t stream);
int ptt_bn_bwd_pooled_sums_f64(const float* dPooled, int ldp, const int32_t* arg, int ns, const float* Z, int ldz, const float* mean,
                               const float* invstd, int R, int C, double* sums, void* workspace, size_t workspace_bytes,
                               const float* act_scale, const float* act_shift, ptt_stream_t stream);
int ptt_bn_bwd_pooled_apply_f32(const float* dPooled, int ldp, const int32_t* arg, int ns, const float* Z, int ldz, const float* mean,
                                const float* invstd, const float* gamma, const float* sum_dy, const float* sum_dy_xhat,
                                const double* count, int R, int C, float* dZ, int ldd, const float* act_scale,
                                const float* act_shift, ptt_stream_t stream);
/* nn.BatchNorm's training-mode bookkeeping in ONE launch (running statistics with momentum, unbiased variance, batch counter);
 * count = the rows the statistics were taken over, a float64 in device memory (SyncBatchNorm: the all-reduced count). */
int ptt_bn_update_running_f32(const float* mean, const float* var, const double* count, float momentum, int C, float* running_mean,
                              float* running_var, int64_t* num_batches_tracked, ptt_stream_t stream);
/* CosineSimAug's first convolution in training mode with its similarity channel split off (p2b_xcoor.py:35-40):
 * z0[b,j,i,:] = P[b,i,:] + cos_t[b,j,i] * w_sim[:]  (rows ordered (b, j, i): search point j, template point i), and its
 * backward in one pass over dz0: dP[b,i,:] = sum_j dz0, dcos[b,j,i] = <dz0[b,j,i,:], w_sim>, dw[:] = sum dz0 * cos_t
 * (fixed summation order). C % 4 == 0; the backward needs C <= 256 (PTT_EINVAL otherwise). */
int ptt_xcorr_z0_f32(const float* P, const float* cos_t, const float* w_sim, int B, int n2, int n1, int C, float* z0, ptt_stream_t stream);
/* the same launch also sums z0's BatchNorm statistics: float64 partials (chunks, 2, C), chunks = ptt_xcorr_z0_stat_chunks(...);
 * at most 1024 channels (PTT_EUNSUPPORTED otherwise, and the chunk query returns 0); fewer than chunks * 2 * C partial_elems:
 * PTT_EWORKSPACE */
int ptt_xcorr_z0_stat_chunks(int B, int n2, int n1, int C);
int ptt_xcorr_z0_stats_f32(const float* P, const float* cos_t, const float* w_sim, int B, int n2, int n1, int C, float* z0,
                           double* stats_partial, size_t partial_elems, ptt_stream_t stream);
/* both backward forms take a workspace of at least ptt_xcorr_z0_bwd_workspace(B, n1, C) bytes (PTT_EWORKSPACE otherwise) */
size_t ptt_xcorr_z0_bwd_workspace(int B, int n1, int C);
/* ptt_xcorr_z0_bwd_f32 when dz0 does not exist yet: G = the gradient w.r.t. relu(BatchNorm(z0)) as ptt_rows_gemm_bnbwd_f32 left it,
 * with that launch's partial sums; layer 0's BatchNorm + ReLU backward is applied while G is read and z0 is recomputed from
 * P / cos / w (neither z0 nor dz0 is read or written). Also returns dgamma / dbeta of that BatchNorm. Same workspace. */
int ptt_xcorr_z0_bnbwd_f32(const double* partial, int chunks, const float* G, const float* P, const float* cos_t, const float* w_sim,
                           const float* mean, const float* invstd, const float* gamma, const float* act_scale, const float* act_shift,
                           int B, int n2, int n1, int C, float* dP, float* dcos, float* dw, float* dgamma, float* dbeta, void* workspace,
                           size_t workspace_bytes, ptt_stream_t stream);
int ptt_xcorr_z0_bwd_f32(const float* dz0, const float* cos_t, const float* w_sim, int B, int n2, int n1, int C, float* dP, float* dcos,
                         float* dw, void* workspace, size_t workspace_bytes, ptt_stream_t stream);
/* Round 3, launch consolidation of the training step (the step is bound by device time, and ~250 of its launches were
 * five-microsecond bookkeeping kernels):
 *   ptt_bn_train_tail   what a training-mode BatchNorm layer does with fresh batch statistics besides normalising
 *     (torch/nn/modules/batchnorm.py; the reference builds the layers in pytorch_utils.py:94-114), written by the SAME
 *     launch that forms the statistics: act_a = gamma * invstd and act_b = beta - mean * act_a (the deferred activation's
 *     constants, each operation rounded separately), running_mean / running_var updated with `momentum` and the n / (n - 1)
 *     variance (n = R), *num_batches_tracked += 1. Null members switch a piece off; a NULL tail = the plain entry point.
 *   ptt_pack_weights_f32  packs n_jobs weights (views by element strides: W[col * stride_out + k * stride_k], so a
 *     transposed pack is a stride swap) into one arena in ONE launch; jobs live in DEVICE memory (a training step re-packs
 *     every weight after each optimiser update: the table is built once, the launch repeats). out_offset: float offset
 *     inside `arena`, a multiple of 4; each job writes ptt_packed_weight_elems(Cout, K) floats.
 *   ptt_sa_z0_rows_f32  the front of one SA level in training mode with layer 0 hoisted, one pass: for row (b, m, k),
 *     n = idx[b,m,k]: rel = (xyz[b,n] - new_xyz[b,m]) (* float(1 / radius) when normalize_xyz, as torch divides by a host
 *     scalar) — QueryAndGroup,
 *     pointnet2_utils.py:350-354 — and z0 = term[b,n,:] + Wx . rel, the first SharedMLP convolution (pytorch_utils.py:12-36;
 *     channel order xyz first, pointnet2_utils.py:359-361) with its feature half `term` (B,N,C) evaluated once per point;
 *     term NULL: a level without point features. z0 (B*M*ns, C) rows, rel_rows (B*M*ns, 3) (the weight gradient of Wx
 *     (C,3), row stride ldw >= 3, needs them). C % 4 == 0, radius > 0 (PTT_EINVAL otherwise); at most (2^31 - 1) / 4 rows per
 *     cloud (PTT_EUNSUPPORTED otherwise). No gradient w.r.t. the coordinates is provided: callers with
 *     learnable coordinates (the box head's vote aggregation) keep ptt_group_f32 + ptt_gather_rows_f32. */
int ptt_sa_z0_rows_f32(const float* xyz, const float* new_xyz, const int32_t* idx, const float* term, const float* wx, int ldw, int B,
                       int N, int M, int ns, int C, float radius, int normalize_xyz, float* z0, float* rel_rows, ptt_stream_t stream);
/* The same launch also summing the BatchNorm statistics of layer 0 (the float64 column sums / sums of squares of z0) as
 * partials (chunks, 2, C), chunks = ptt_sa_z0_rows_stat_chunks(B, M, ns, C), for ptt_bn_finish_partials_f32 (or its _train form) — no
 * statistics pass over z0. C <= 1024 (PTT_EUNSUPPORTED otherwise, and the chunk query returns 0). */
int ptt_sa_z0_rows_stat_chunks(int B, int M, int ns, int C);
int ptt_sa_z0_rows_stats_f32(const float* xyz, const float* new_xyz, const int32_t* idx, const float* term, const float* wx, int ldw, int B,
                             int N, int M, int ns, int C, float radius, int normalize_xyz, float* z0, float* rel_rows,
                             double* stats_partial, size_t partial_elems, ptt_stream_t stream);
typedef struct ptt_bn_train_tail {
    const float* gamma; const float* beta;      /* (C) affine parameters, needed for act_a / act_b */
    float* act_a; float* act_b;                 /* (C) out, or both NULL */
    float* running_mean; float* running_var;    /* (C) updated in place, or both NULL */
    int64_t* num_batches_tracked;               /* incremented, or NULL */
    float momentum;
} ptt_bn_train_tail;
int ptt_bn_stats_train_f32(const float* X, int R, int C, int ldx, float eps, float* mean, float* var, float* invstd,
                           void* workspace, size_t workspace_bytes, const ptt_bn_train_tail* tail, ptt_stream_t stream);
int ptt_bn_finish_partials_train_f32(const double* partial, int chunks, int C, int R, float eps, float* mean, float* var,
                                     float* invstd, const ptt_bn_train_tail* tail, ptt_stream_t stream);
typedef struct ptt_pack_job {
    const float* W;
    int64_t out_offset, stride_out, stride_k;
    int32_t Cout, K;
} ptt_pack_job;
int ptt_pack_weights_f32(const ptt_pack_job* jobs_device, int n_jobs, float* arena, ptt_stream_t stream);
size_t ptt_linear_wgrad2_workspace(int R, int Cout, int Cin);
int ptt_linear_wgrad2_f32(const float* dZ, int ldz, const float* X, int ldx, int R, int Cout, int Cin, float* dW,
                          int accumulate, void* workspace, size_t workspace_bytes, const float* x_scale, const float* x_shift,
                          ptt_stream_t stream);

/* The four tracking losses of a training step with their gradients, in two launches (reference
 * ptt/models/voting_heads/centroids_voting_head.py:29-62: BCEWithLogits (mean) over the seed scores + masked smooth-L1 of the votes;
 * box_voting_head.py:33-66: masked BCEWithLogits of the proposal scores + label-weighted smooth-L1 of the 4 box numbers; the
 * proposal labels / masks of box_voting_head.py:96-104 are formed in the kernels from the proposal centres).
 *   seed_cls (B,N) logits; cls_label (B,Ns) per search POINT with search_inds (B,N) int64 the seeds' point indices, or
 *   search_inds NULL and cls_label (B,N) per seed; votes (B,N,3); reg_label (B, ld_reg >= 4): gt centre + angle;
 *   box_data (B,M,5) = (x, y, z, angle, score logit); centres (B,M,3); pos_weight_*: device scalars (the modules' buffers).
 * out8: [0] the weighted total, [1..4] the un-weighted losses (seed cls, seed reg, proposal cls, proposal reg), [5..7] the sums
 * of the seed labels / proposal masks / proposal labels (the backward's denominators). Reductions in float64, fixed order.
 * ptt_track_losses_bwd_f32: d total / d (seed_cls, votes, box_data) times upstream[0] (device scalar; NULL: 1). */
typedef struct ptt_track_loss_desc {
    const float* seed_cls;
    const float* cls_label;
    const int64_t* search_inds;
    const float* votes;
    const float* reg_label;
    const float* box_data;
    const float* centres;
    const float* pos_weight_seed;
    const float* pos_weight_box;
    int32_t B, N, Ns, M, ld_reg;
    float w_seed_cls, w_seed_reg, w_box_cls, w_box_reg;
} ptt_track_loss_desc;
int ptt_track_losses_f32(const ptt_track_loss_desc* desc, float* out8, float* total /* optional: out8[0] once more */, ptt_stream_t stream);
int ptt_track_losses_bwd_f32(const ptt_track_loss_desc* desc, const float* out8, const float* upstream, float* d_seed_cls,
                             float* d_votes, float* d_box_data, ptt_stream_t stream);
/* torch.nn.utils.clip_grad_norm_(params, max_norm) + torch.optim.Adam.step() (tools/train_utils/train_utils.py:48-51,
 * optimization/__init__.py:12-14) over a device table of tensors in two launches. The caller cuts every tensor into chunks of
 * ptt_adam_chunk_elems() elements: chunk_tensor[w] = table index, chunk_first[w] = first element. hyper: step_size =
 * lr / (1 - beta1^t), bias2_sqrt = sqrt(1 - beta2^t); max_norm <= 0: no clipping (partial may be NULL); write_clipped: also
 * scale .grad in place as clip_grad_norm_ leaves it. partial: n_chunks doubles of workspace; norm_out (optional): the total norm. */
typedef struct ptt_adam_tensor {
    float* param;
    float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t n;
} ptt_adam_tensor;
typedef struct ptt_adam_hyper {
    float beta1, beta2, one_minus_beta1, one_minus_beta2 /* formed in double by the caller, as torch does */, eps, step_size, bias2_sqrt,
          weight_decay, max_norm;
    int32_t write_clipped;
} ptt_adam_hyper;
int ptt_adam_chunk_elems(void);
int ptt_adam_clip_step_f32(const ptt_adam_tensor* tensors_device, const int32_t* chunk_tensor_device, const int64_t* chunk_first_device,
                           int n_chunks, const ptt_adam_hyper* hyper, double* partial, size_t partial_elems, float* norm_out,
                           ptt_stream_t stream);
/* The same two launches with the hyper-parameters read from DEVICE memory when the update launch runs: the form a captured
 * training step (hipGraph) replays, the host writing step_size / bias2_sqrt (and a scheduler's lr) of the step into hyper_device
 * before each replay. clip != 0: the norm pass is launched and hyper_device->max_norm (> 0) clips; clip == 0: hyper_device->max_norm
 * must be <= 0. Arithmetic identical to ptt_adam_clip_step_f32. */
int ptt_adam_clip_step_dev_f32(const ptt_adam_tensor* tensors_device, const int32_t* chunk_tensor_device, const int64_t* chunk_first_device,
                               int n_chunks, const ptt_adam_hyper* hyper_device, int clip, double* partial, size_t partial_elems,
                               float* norm_out, ptt_stream_t stream);
/* The same step for every optimizer of the reference's OPTIMIZATION block (tools/train_utils/optimization/__init__.py:11-39):
 * clip_grad_norm_(ALL parameters, max_norm) + optimizer.step() over a table whose rows carry a GROUP index into an array of
 * per-group hyper-parameters. ONE norm is formed over every row of every group (what clip_grad_norm_(model.parameters(), ..)
 * in front of optimizer.step() computes); chunking, the float64 partial sums combined in a fixed order and
 * clip = min(1, max_norm / (norm + 1e-6)) are those of ptt_adam_clip_step_f32. hyper[g].kind, with g' = clip g:
 *   PTT_OPTIM_ADAM   torch.optim.Adam: g' += weight_decay p (L2), then the update of ptt_adam_clip_step_f32, bit for bit
 *   PTT_OPTIM_ADAMW  torch.optim.AdamW (= OptimWrapper.step with true_wd, fastai_optim.py:132-149): p *= decay, decay =
 *                    1 - lr weight_decay formed in double by the caller; then the Adam update without the L2 term
 *   PTT_OPTIM_SGD    torch.optim.SGD, dampening 0, no nesterov: g' += weight_decay p; buf = g' when first_step != 0 and
 *                    beta1 buf + g' otherwise (beta1 = the momentum); p += (-step_size) buf, step_size = lr. beta1 == 0: no
 *                    buffer, state1 may be NULL and p += (-step_size) g'
 * state1 = exp_avg | momentum_buffer, state2 = exp_avg_sq | NULL. step_size / bias2_sqrt as in ptt_adam_hyper, per group (groups
 * may stand at different step counts). max_norm <= 0: no clipping (partial may be NULL); write_clipped: .grad *= clip in place.
 * Refused with PTT_EINVAL, nothing launched: a null table or hyper, n_groups < 1 (more than PTT_OPTIM_MAX_GROUPS: PTT_EUNSUPPORTED), an unknown kind, an
 * Adam kind with bias2_sqrt <= 0 or eps < 0; and, when tensors_host (optional: the host copy of the n_tensors rows the device
 * table was uploaded from) is given, a row whose group lies outside [0, n_groups), whose param / grad is null, or an SGD row
 * with beta1 != 0 and a null state1, an Adam row with a null state. PTT_EWORKSPACE: clipping with partial_elems < n_chunks. */
#define PTT_OPTIM_ADAM 0
#define PTT_OPTIM_ADAMW 1
#define PTT_OPTIM_SGD 2
#define PTT_OPTIM_MAX_GROUPS 8
typedef struct ptt_optim_tensor {
    float* param;
    float* grad;
    float* state1;
    float* state2;
    int64_t n;
    int32_t group, reserved;
} ptt_optim_tensor;
typedef struct ptt_optim_hyper {
    int32_t kind, first_step;
    float beta1, beta2, one_minus_beta1, one_minus_beta2, eps, step_size, bias2_sqrt, weight_decay, decay;
    int32_t reserved;
} ptt_optim_hyper;
int ptt_optim_clip_step_f32(const ptt_optim_tensor* tensors_device, const ptt_optim_tensor* tensors_host, int n_tensors,
                            const int32_t* chunk_tensor_device, const int64_t* chunk_first_device, int n_chunks,
                            const ptt_optim_hyper* hyper, int n_groups, float max_norm, int write_clipped, double* partial,
                            size_t partial_elems, float* norm_out, ptt_stream_t stream);
/* The same two launches with the n_groups hyper-parameter entries read from DEVICE memory when the update launch runs: the form
 * a captured training step replays, the host writing every group's entry (a OneCycle schedule moves lr and beta1 on every step)
 * into hyper_device before each replay. max_norm and write_clipped are launch arguments: a capture fixes them. The entries
 * cannot be seen here, so only the table (tensors_host: group range, null param / grad), n_groups and the workspace are checked;
 * a row the update launch finds unusable (group out of range, unknown kind, a state its kind needs is null) is left untouched.
 * Arithmetic identical to ptt_optim_clip_step_f32. */
int ptt_optim_clip_step_dev_f32(const ptt_optim_tensor* tensors_device, const ptt_optim_tensor* tensors_host, int n_tensors,
                                const int32_t* chunk_tensor_device, const int64_t* chunk_first_device, int n_chunks,
                                const ptt_optim_hyper* hyper_device, int n_groups, float max_norm, int write_clipped, double* partial,
                                size_t partial_elems, float* norm_out, ptt_stream_t stream);
/* The step ledger: one launch (one workgroup, one wave) appends one row of a training step's scalars to a ring in device memory
 * and updates running statistics — what the reference's loop reads back with loss.item() and four tb_dict values on every step
 * (tools/train_utils/train_utils.py:54-70), without a host read. Capturable: no host reads, no allocation; ordered by the stream
 * alone (no atomics), so it is recorded behind the optimizer's update of a captured step.
 *   losses: the first five floats of ptt_track_losses_f32's out8 = [total, seed cls, seed reg, proposal cls, proposal reg]
 *   norm:   the optimizer's norm_out (one float), or NULL: column 5 is then written as 0 and takes no part in the finiteness test
 *   ring:   (capacity, PTT_LEDGER_COLS) float32; row k (counted from 0 over the ledger's life) goes to slot k % capacity, bit for bit
 *   counts: int64[2] = {appended: rows ever appended; non_finite: rows with an inf / NaN among the provided columns}
 *   sums:   double[PTT_LEDGER_COLS]: per column, the sum over the FINITE rows only, added in append order by one lane per column
 *           (a host loop `s += (double)x` over those rows reproduces it bit for bit)
 * counts and sums start from what the caller put there (zeros). PTT_EINVAL, nothing launched: losses == NULL, capacity < 1, a
 * null ring / counts / sums. */
#define PTT_LEDGER_COLS 6
int ptt_step_ledger_f32(const float* losses, const float* norm, float* ring, long long capacity, int64_t* counts, double* sums,
                        ptt_stream_t stream);
/* The two element-wise ends of CosineSimAug's cosine map in training (p2b_xcoor.py:35-42 via nn.CosineSimilarity); the map
 * itself is a batched product of unit rows.
 *   ptt_unit_rows_f32     x addressed as x[b * sb + j * sn + c * sc] (any layout) -> unit (B,n,C) rows x / max(|x|, eps) and
 *                         nrm (B,n) = max(|x|, eps), stored NEGATIVE where the clamp is active
 *   ptt_cos_bwd_rows_f32  dx[b,j,:] = (A[b,j,:] - (sum_i G[b,j,i] cos[b,j,i]) unit[b,j,:]) / |nrm[b,j]| (no projection term where
 *                         nrm < 0), A (B,n,C) = the caller's product of G with the OTHER side's unit rows; G / cos addressed as
 *                         [b * map_sb + j * own + i * other], i < m; dx written as dx[b * sb + j * sn + c * sc] */
int ptt_unit_rows_f32(const float* x, long long sb, long long sn, long long sc, int B, int n, int C, float eps, float* unit, float* nrm,
                      ptt_stream_t stream);
int ptt_cos_bwd_rows_f32(const float* A, const float* unit, const float* nrm, const float* G, const float* cosm, long long map_sb,
                         long long own, long long other, int m, int B, int n, int C, float* dx, long long sb, long long sn, long long sc,
                         ptt_stream_t stream);
/* Layer 0 of a hoisted SA level, backward, in one pass in row order over the gradient G (R, C) of its ACTIVATED output (training):
 * the BatchNorm + ReLU backward is applied row by row from G, the stored z0 and the sums of `partial` (ptt_rows_gemm_bnbwd_f32's),
 * dwx (C,3) = dz0^T rel_rows is accumulated on the way, and dz0 is written only if dz_out != NULL (a level with point features:
 * its row scatter reads it; dz_out may alias G). Also dgamma / dbeta of that BatchNorm. dwx NULL: the partial sums of dwx,
 * [workspace bytes / (12 C)][C][3], stay in the workspace for ptt_grad_finish_f32. */
size_t ptt_sa_z0_bnbwd_workspace(long long R, int C);
int ptt_sa_z0_bnbwd_f32(const double* partial, int chunks, const float* G, const float* Z0, const float* rel_rows, const float* mean,
                        const float* invstd, const float* gamma, const float* act_scale, const float* act_shift, long long R, int C,
                        float* dz_out, float* dwx, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, ptt_stream_t stream);

/* The parameter gradients of a training step finished by ONE launch (reference tools/train_utils/train_utils.py:47-49:
 * loss.backward() has every .grad complete before clip_grad_norm_ reads it; tools/train_tracking.py:158-159: the gradient that
 * DistributedDataParallel averages over ranks). The *_partials entries are ptt_linear_wgrad_f32 / ptt_linear_wgrad2_f32 /
 * ptt_colsum_f32 without their finishing launch: the row-chunk partial sums [*nchunks][Cout * Cin] (resp. [*nchunks][C]) stay in
 * `workspace` (same size queries). ptt_grad_finish_f32 then adds, for every SEGMENT (one destination inside the flat float32
 * gradient buffer `flat`: n elements as rows of `cols`, row stride `ld`, first element `dst`; 16-byte aligned pieces when `vec`),
 * the chunks of its jobs [job0, job0 + njobs) in a fixed order; `out` (a power of two, 4 ... 256) = outputs per workgroup, the
 * other 256 / out thread groups split the chunks. blocks_device: pairs (segment, first output unit) per workgroup; a unit is
 * 4 elements of a vec segment, else 1. Every job of a segment holds partials of that segment's n. Tables live on the device. */
typedef struct ptt_grad_job {
    const float* partial;
    int32_t nchunks, reserved;
} ptt_grad_job;
typedef struct ptt_grad_segment {
    int64_t dst;
    int32_t n, cols, ld, job0, njobs, out, vec, reserved;
} ptt_grad_segment;
int ptt_linear_wgrad_partials_f32(const float* dZ, int ldz, const float* X, int ldx, int R, int Cout, int Cin, void* workspace,
                                  size_t workspace_bytes, const float* x_scale, const float* x_shift, int* nchunks, ptt_stream_t stream);
int ptt_linear_wgrad2_partials_f32(const float* dZ, int ldz, const float* X, int ldx, int R, int Cout, int Cin, void* workspace,
                                   size_t workspace_bytes, const float* x_scale, const float* x_shift, int* nchunks, ptt_stream_t stream);
int ptt_colsum_partials_f32(const float* X, int R, int C, int ldx, void* workspace, size_t workspace_bytes, int* nchunks,
                            ptt_stream_t stream);
int ptt_grad_finish_f32(const ptt_grad_segment* segments_device, const ptt_grad_job* jobs_device, const int32_t* blocks_device,
                        int n_blocks, float* flat, ptt_stream_t stream);

/* The backward pass of a Point-Transformer block's attention core (variants.py:158-163 under autograd) with three passes folded away:
 *   ptt_rows_gemm_rsum16_f32     plain = X @ W^T, out = plain + residual and, per group of 16 consecutive rows (a point's 16
 *                                neighbours), gsum[g, :] = the column sums of plain over the group — one epilogue. With X = the gradient
 *                                of fc_gamma's hidden layer and residual = the aggregation's gradient of (v + pos_enc): plain is the
 *                                gradient of the pair input, out the gradient of pos_enc (its two consumers' sum, which autograd would
 *                                form with a pass of its own) and gsum the gradient of q (a reduction pass).
 *                                ptt_rows_gemm_rsum16_supported: K % 128 == 0, N % 128 == 0, rows % 16 == 0.
 *   ptt_scatter_rows_csr_sub_f32 ptt_scatter_rows_csr_f32 with out = minuend - (the sums), minuend NULL = 0: the gradient of k is
 *                                MINUS the scatter of the pair input's gradient (a negation pass). */
int ptt_rows_gemm_rsum16_supported(int rows, int K, int N, int ldx);
int ptt_rows_gemm_rsum16_f32(const float* X, int rows, int K, int ldx, const float* Wpacked, int N, const float* residual, int ldr,
                             float* out, int ldo, float* plain, int ldp, float* gsum, int ldg, ptt_stream_t stream);
int ptt_scatter_rows_csr_sub_f32(const float* g, const int32_t* order, const int32_t* start, int B, int N, int E, int C,
                                 const float* minuend, float* out, ptt_stream_t stream);

/* ---------------------------------------------------------------------------------
 * MulTransformerBlock in TRAINING mode (transformer_block/multitransformer.py:37-63 under autograd), ABI 25:
 *   ptt_layernorm_train_fwd_f32  out = LayerNorm_C(x) * weight + bias (+ residual) over the rows of a (rows, C) matrix as
 *                                ptt_layernorm_f32 (one wave per row, biased variance of the centred values, eps inside the root),
 *                                and the row's mean and rstd = 1 / sqrt(var + eps) (float32, `rows` each) for the backward pass.
 *                                C <= 1024; weight and bias are required.
 *   ptt_layernorm_bwd_f32        with g = dy * weight, xhat = (x - mean) * rstd:
 *                                  dx = rstd * (g - mean_c(g) - xhat * mean_c(g * xhat))      one wave per row
 *                                  dbias = sum_rows dy, dweight = sum_rows dy * xhat          fixed 32-row chunks -> float64 partial
 *                                slabs in the workspace -> a finish in chunk order: no atomics, bit-reproducible. The residual's
 *                                gradient is dy itself. workspace: ptt_layernorm_bwd_workspace(rows, C) bytes.
 *   ptt_rows_gemm_rsum16_heads_f32   ptt_rows_gemm_rsum16_f32 for fc_gamma[0] of a block with D / hd heads: X (rows, D) is head-major
 *                                in the channel axis (channel c = h * hd + d), Wpacked ONE hd x hd weight all heads share, and
 *                                plain[:, h hd : (h + 1) hd] = X[:, h hd : (h + 1) hd] @ W^T; out and gsum as the single-head form.
 *                                ptt_rows_gemm_rsum16_heads_supported: D % hd == 0, hd % 128 == 0, D % 128 == 0, rows % 16 == 0.
 * ------------------------------------------------------------------------------- */
int ptt_layernorm_train_fwd_f32(const float* x, int rows, int C, int ldx, const float* weight, const float* bias, float eps,
                                const float* residual, int ldr, float* out, int ldo, float* mean, float* rstd, ptt_stream_t stream);
size_t ptt_layernorm_bwd_workspace(int rows, int C);
int ptt_layernorm_bwd_f32(const float* dy, int ldg, const float* x, int ldx, const float* mean, const float* rstd, const float* weight,
                          int rows, int C, float* dx, int ldd, float* dweight, float* dbias, void* workspace, size_t workspace_bytes,
                          ptt_stream_t stream);
int ptt_rows_gemm_rsum16_heads_supported(int rows, int D, int hd, int ldx);
int ptt_rows_gemm_rsum16_heads_f32(const float* X, int rows, int D, int hd, int ldx, const float* Wpacked, const float* residual, int ldr,
                                   float* out, int ldo, float* plain, int ldp, float* gsum, int ldg, ptt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PTT_HIP_H */

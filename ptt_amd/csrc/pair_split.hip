// Split-bf16 form of the single-head Point-Transformer pair kernel (gfx950): ptt_pt_attn_pair_split_f32 and the weight
// split + pack it reads, ptt_pack_weight_split_bf16. The opt-in arithmetic of TransformerBlock.precision = 'bf16x2'.
//
// Arithmetic. Every fp32 operand x of the block's three D x D GEMMs (fc_delta[2], fc_gamma[0], fc_gamma[2]) is written as
// two bf16 pieces, hi = bf16(x) (round to nearest even) and lo = bf16(x - float(hi)), and a product a . w becomes
//     a_hi . w_hi + a_hi . w_lo + a_lo . w_hi          (three v_mfma_f32_32x32x16_bf16 into ONE fp32 accumulator);
// the dropped a_lo . w_lo term and the two lo roundings are each <= 2^-16 |a| |w| per product (typically 2^-18). Everything else is the fp32
// kernel's (pt_attn_pair_body.h): rel rows and fc_delta[0] as one exact fp32 K-block, q / k / v read as fp32, biases,
// softmax, weighted sum and the stores in fp32, fc_gamma[2].bias never read.
//
// Geometry: that of pt_attn_pair_kernel<D, KNN> — a 32-row tile of 32 / KNN whole points, 4 waves x D / 128 column tiles,
// the same phases and barriers. The C/D layout of 32x32x16_bf16 is the one tile_row() describes, so the epilogues, the
// max_halves / add_halves softmax and the stores carry over unchanged.
//
// LDS image: the A operand is two bf16 planes Xh, Xl of [32][D + 8]. Lane l reads row l & 31, elements 16 kb + 8 (l >> 5)
// .. + 7 of a plane with one ds_read_b128; the row stride of (D + 8) / 2 dwords is 4 mod 8, i.e. one 16-byte bank group
// further per row, so the 16 lanes that share an LDS cycle hit 16 distinct groups (the rule the fp32 tile's D + 4 floats
// follow). The epilogue that writes the next layer's input splits its fp32 value and stores the two pieces along the
// accumulator layout (column on the lane, 16 rows in the registers).
//
// Weights: ptt_pack_weight_split_bf16's order (include/ptt_hip.h) — per (16-channel block, 32-column tile, piece) one
// 1 KiB fragment, lane l's 8 elements = one 16-byte buffer load; a K-block costs a wave 2 CT loads, as many bytes as the
// two fp32 K-blocks it replaces. One block is prefetched across every epilogue, as in the fp32 body.
#include <math.h>
#include "common.h"
#include "mfma_common.h"

namespace ptt {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// Per-phase cycle stamps (scripts/pair_phases.py): only in -DPTT_DEV builds, as in mfma_ops.hip.
#ifdef PTT_DEV
#define PTT_STAMP(i) do { if (p.dbg && threadIdx.x == 0 && blockIdx.x < 4096) p.dbg[blockIdx.x * 8 + (i)] = __builtin_readcyclecounter(); } while (0)
#else
#define PTT_STAMP(i) do { } while (0)
#endif

// mfma_ops.hip's stagger_second_slot, restated: the workgroup on a CU's second LDS allocation starts `quanta` x ~8k cycles late
// in the first wave of workgroups (speed only).
__device__ __forceinline__ void split_stagger_second_slot(int first_wave_blocks, int quanta) {
    if ((int)blockIdx.x < first_wave_blocks && quanta > 0) {
        const unsigned alloc = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 6);   // HW_REG_LDS_ALLOC
        const unsigned lds_base = alloc & 0xffu, lds_size = (alloc >> 12) & 0x1ffu;
        int slot = lds_size ? (int)(lds_base / lds_size) : 0;
        if (lds_base != 0 && slot == 0) slot = 1;
        for (int i = 0; i < slot * quanta; ++i) __builtin_amdgcn_s_sleep(127);
    }
}

// ------------------------------------------------------------------------------------------
// weight split + pack
// ------------------------------------------------------------------------------------------
// bf16(x), round to nearest even, on the bits (finite x)
__host__ __device__ __forceinline__ unsigned bf16_rne_bits(float x) {
    const unsigned u = __builtin_bit_cast(unsigned, x);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// element e = (((kb * NT + ct) * 2 + piece) * 64 + lane) * 8 + j  holds piece of W[32 ct + (lane & 31)][16 kb + 8 (lane >> 5) + j]
__global__ __launch_bounds__(256) void pack_weight_split_kernel(const float* __restrict__ W, int K, int NT, size_t total,
                                                                unsigned short* __restrict__ P) {
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(e & 7);
        const int lane = (int)((e >> 3) & 63);
        const int piece = (int)((e >> 9) & 1);
        const size_t tile = e >> 10;
        const int ct = (int)(tile % NT);
        const int kb = (int)(tile / NT);
        const float w = W[(size_t)(ct * 32 + (lane & 31)) * K + kb * 16 + 8 * (lane >> 5) + j];
        const unsigned hi = bf16_rne_bits(w);
        const float lo = w - __builtin_bit_cast(float, hi << 16);
        P[e] = (unsigned short)(piece ? bf16_rne_bits(lo) : hi);
    }
}

// ------------------------------------------------------------------------------------------
// the kernel
// ------------------------------------------------------------------------------------------
struct AttnSplitParams {
    const float* xyz; const float* rel; const int32_t* knn; const float* qkv; const float* Wd1p;
    const void* Wd2s; const float* bd2; const void* Wg1s; const float* bg1; const void* Wg2s;
    float* res; float* attn;
    const int32_t* order;
    int BN, N, first_wave, stagger;
    long long* dbg;
};

// hi / lo pieces of x at Xh[i] / Xl[i]
__device__ __forceinline__ void put_split(unsigned short* Xh, unsigned short* Xl, int i, float x) {
    const __bf16 h = (__bf16)x;
    const __bf16 l = (__bf16)(x - (float)h);
    Xh[i] = __builtin_bit_cast(unsigned short, h);
    Xl[i] = __builtin_bit_cast(unsigned short, l);
}

__device__ __forceinline__ int split_wvoff(int w, int lane) { return (w * 128 + lane) * 16; }   // tile w, piece 0, this lane

// First K-block of a split pack for this wave's CT column tiles w, w + 4, ..: pre[2 u + piece]
template <int CT>
__device__ __forceinline__ void prefetch_split(const void* Ws, int w, int lane, f32x4 (&pre)[2 * CT]) {
    const __amdgpu_buffer_rsrc_t wr = weight_rsrc(Ws);
    const int voff = split_wvoff(w, lane);
#pragma unroll
    for (int i = 0; i < 2 * CT; ++i) pre[i] = weight_load(wr, voff, (i >> 1) * 8192 + (i & 1) * 1024);
}

template <int CT>
__device__ __forceinline__ void split_block(const unsigned short* ah_p, const unsigned short* al_p, const f32x4 (&b)[2 * CT],
                                            f32x16 (&acc)[1][CT]) {
    const bf16x8 ah = *reinterpret_cast<const bf16x8*>(ah_p);
    const bf16x8 al = *reinterpret_cast<const bf16x8*>(al_p);
#pragma unroll
    for (int u = 0; u < CT; ++u)
        acc[0][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, __builtin_bit_cast(bf16x8, b[2 * u]), acc[0][u], 0, 0, 0);
#pragma unroll
    for (int u = 0; u < CT; ++u)
        acc[0][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, __builtin_bit_cast(bf16x8, b[2 * u + 1]), acc[0][u], 0, 0, 0);
#pragma unroll
    for (int u = 0; u < CT; ++u)
        acc[0][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, __builtin_bit_cast(bf16x8, b[2 * u]), acc[0][u], 0, 0, 0);
}

// acc[0][u] += X[32 rows][0:D] . W[:, column tile w + 4 u]^T in two-piece arithmetic. One block of weights in flight, the
// last block peeled so that the loop body has no conditional load (gemm_core's PF = 1 form).
template <int D>
__device__ __forceinline__ void gemm_split(const unsigned short* Xh, const unsigned short* Xl, int lda, const void* Ws, int w, int lane,
                                           f32x16 (&acc)[1][D / 128], const f32x4 (&pre)[2 * (D / 128)]) {
    constexpr int CT = D / 128, NT = D / 32, NKB = D / 16;
    const int aoff = (lane & 31) * lda + 8 * (lane >> 5);
    const unsigned short* ah = Xh + aoff;
    const unsigned short* al = Xl + aoff;
    const __amdgpu_buffer_rsrc_t wr = weight_rsrc(Ws);
    const int voff = split_wvoff(w, lane);
    constexpr int wkstep = NT * 2048;                       // bytes per K-block: NT tiles x 2 pieces x 1 KiB
    f32x4 bcur[2 * CT], bnxt[2 * CT];
#pragma unroll
    for (int i = 0; i < 2 * CT; ++i) { bcur[i] = pre[i]; bnxt[i] = bcur[i]; }
    for (int kb = 0; kb + 1 < NKB; ++kb) {
#pragma unroll
        for (int i = 0; i < 2 * CT; ++i) bnxt[i] = weight_load(wr, voff, (kb + 1) * wkstep + (i >> 1) * 8192 + (i & 1) * 1024);
        split_block<CT>(ah + kb * 16, al + kb * 16, bcur, acc);
#pragma unroll
        for (int i = 0; i < 2 * CT; ++i) bcur[i] = bnxt[i];
    }
    split_block<CT>(ah + (NKB - 1) * 16, al + (NKB - 1) * 16, bcur, acc);
}

template <int D, int KNN>
__global__ __launch_bounds__(256, 2) void pt_attn_pair_split_kernel(AttnSplitParams p) {
    static_assert(KNN == 8 || KNN == 16 || KNN == 32, "a 32-row tile splits into whole points");
    static_assert(D % 128 == 0, "4 waves x 32 columns per column-tile round");
    constexpr int NT = D / 32, CT = NT / 4, LDA = D + 8;
    constexpr int PTS = 32 / KNN, G = KNN / 2;
    extern __shared__ __attribute__((aligned(16))) unsigned short smem_h[];
    unsigned short* Xh = smem_h;                                         // [32][LDA] bf16, hi pieces
    unsigned short* Xl = smem_h + 32 * LDA;                              // [32][LDA] bf16, lo pieces
    int* nb = reinterpret_cast<int*>(smem_h + 64 * LDA);                 // [32] byte offset of the neighbour's q|k|v row
    constexpr int LDR = 12;                                              // [rel.x rel.y rel.z 1 | 0 0 0 0] + pad
    float* relt = reinterpret_cast<float*>(nb + 32);                     // [32][LDR] fp32: the A operand of fc_delta[0]
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, half = lane >> 5;
    const int slot0 = logical_block() * PTS;
    const int npts = min(PTS, p.BN - slot0);
#define PTT_SLOT(i) (slot0 + (i) < p.BN ? slot0 + (i) : p.BN - 1)
    const int s0 = slot0 < p.BN ? slot0 : p.BN - 1, s1 = PTS > 1 ? PTT_SLOT(1) : s0;
    const int s2 = PTS > 2 ? PTT_SLOT(2) : s0, s3 = PTS > 2 ? PTT_SLOT(3) : s0;
#undef PTT_SLOT
    const int pt0 = p.order ? p.order[s0] : s0, pt1 = PTS > 1 ? (p.order ? p.order[s1] : s1) : pt0;
    const int pt2 = PTS > 2 ? (p.order ? p.order[s2] : s2) : pt0, pt3 = PTS > 2 ? (p.order ? p.order[s3] : s3) : pt0;
    const int pt[4] = {pt0, pt1, pt2, pt3};                 // indexed by unrolled loop counters only
    f32x4 pre1[CT];
    {                                                       // fc_delta[0]'s only weight block (fp32 pack): requested first
        const f32x4* bp = reinterpret_cast<const f32x4*>(p.Wd1p) + (size_t)w * 64 + lane;
#pragma unroll
        for (int u = 0; u < CT; ++u) pre1[u] = bp[(size_t)u * 4 * 64];
    }
    split_stagger_second_slot(p.first_wave, p.stagger);
    PTT_STAMP(0);

    if (t < 32) {
        // row t: point t / KNN of the tile, neighbour t % KNN
        const int me = PTS == 1 ? pt0 : PTS == 2 ? ((t >> 4) ? pt1 : pt0) : ((t >> 4) ? ((t & 8) ? pt3 : pt2) : ((t & 8) ? pt1 : pt0));
        const int b = me / p.N;
        const int n = p.knn[(size_t)me * KNN + (t & (KNN - 1))];
        const int flat = b * p.N + n;
        nb[t] = n * (3 * D * (int)sizeof(float));
        f32x4 r4;
        if (p.rel) {
            const float* rl = p.rel + ((size_t)me * KNN + (t & (KNN - 1))) * 3;
            r4 = f32x4{rl[0], rl[1], rl[2], 1.f};
        } else {
            r4 = f32x4{p.xyz[(size_t)me * 3 + 0] - p.xyz[(size_t)flat * 3 + 0],
                       p.xyz[(size_t)me * 3 + 1] - p.xyz[(size_t)flat * 3 + 1],
                       p.xyz[(size_t)me * 3 + 2] - p.xyz[(size_t)flat * 3 + 2], 1.f};
        }
        *reinterpret_cast<f32x4*>(relt + t * LDR) = r4;
        *reinterpret_cast<f32x4*>(relt + t * LDR + 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    lds_barrier();

    int cols[CT];
#pragma unroll
    for (int u = 0; u < CT; ++u) cols[u] = (w + 4 * u) * 32 + (lane & 31);

    f32x4 pre[2 * CT];
    // fc_delta[0] + ReLU: h = relu([rel 1] . [W | b]^T) as ONE exact fp32 K-block (K = 4, zero-padded to 8), as in the fp32 kernel
    {
        f32x16 h[CT];
        const f32x4 a = *reinterpret_cast<const f32x4*>(relt + (lane & 31) * LDR + 4 * half);
#pragma unroll
        for (int u = 0; u < CT; ++u) {
#pragma unroll
            for (int r = 0; r < 16; ++r) h[u][r] = 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int u = 0; u < CT; ++u) h[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], pre1[u][j], h[u], 0, 0, 0);
        prefetch_split<CT>(p.Wd2s, w, lane, pre);           // fc_delta[2]'s first weight block
#pragma unroll
        for (int u = 0; u < CT; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) put_split(Xh, Xl, tile_row(r, half) * LDA + cols[u], fmaxf(h[u][r], 0.f));
    }
    lds_barrier();

    PTT_STAMP(1);
    // ---- delta = fc_delta[2](h) ----
    f32x16 delta[1][CT];
#pragma unroll
    for (int u = 0; u < CT; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) delta[0][u][r] = 0.f;
    gemm_split<D>(Xh, Xl, LDA, p.Wd2s, w, lane, delta, pre);
    prefetch_split<CT>(p.Wg1s, w, lane, pre);               // next GEMM's first block: in flight across the epilogue
#pragma unroll
    for (int u = 0; u < CT; ++u) {
        const float bb = p.bd2[cols[u]];
#pragma unroll
        for (int r = 0; r < 16; ++r) delta[0][u][r] += bb;
    }
    PTT_STAMP(2);
    // gathers of neighbour k / v rows: raw buffer loads on a descriptor based at the cloud's first q|k|v row
    const int cloud = pt[0] / p.N;
    const __amdgpu_buffer_rsrc_t rq = weight_rsrc(p.qkv + (size_t)cloud * p.N * 3 * D);
    int nrow[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) nrow[r] = nb[tile_row(r, half)] + (w * 32 + (lane & 31)) * (int)sizeof(float);

    lds_barrier();  // all waves done with h
    // t = (q_i - k_j) + delta  -> X
    {
        const int pa = pt0, pb = (npts > 1) ? pt1 : pt0, pc = (npts > 2) ? pt2 : pt0, pd = (npts > 3) ? pt3 : pt0;
#pragma unroll
        for (int u = 0; u < CT; ++u) {
            const float qa = p.qkv[(size_t)pa * 3 * D + cols[u]];
            const float qb = PTS > 1 ? p.qkv[(size_t)pb * 3 * D + cols[u]] : qa;
            const float qc = PTS > 2 ? p.qkv[(size_t)pc * 3 * D + cols[u]] : qa;
            const float qd = PTS > 2 ? p.qkv[(size_t)pd * 3 * D + cols[u]] : qa;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float kv = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                    rq, nrow[r] + (D + u * 128) * (int)sizeof(float), 0, 0));
                const float q = PTS == 1 ? qa : PTS == 2 ? ((r < 8) ? qa : qb) : ((r < 8) ? ((r < 4) ? qa : qb) : ((r < 12) ? qc : qd));
                put_split(Xh, Xl, tile_row(r, half) * LDA + cols[u], (q - kv) + delta[0][u][r]);
            }
        }
    }
    lds_barrier();

    PTT_STAMP(3);
    // ---- g = relu(fc_gamma[0](t)) -> X ----
    {
        f32x16 acc[1][CT];
#pragma unroll
        for (int u = 0; u < CT; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[0][u][r] = 0.f;
        gemm_split<D>(Xh, Xl, LDA, p.Wg1s, w, lane, acc, pre);
        prefetch_split<CT>(p.Wg2s, w, lane, pre);
        PTT_STAMP(4);
        lds_barrier();
#pragma unroll
        for (int u = 0; u < CT; ++u) {
            const float bb = p.bg1[cols[u]];
#pragma unroll
            for (int r = 0; r < 16; ++r) put_split(Xh, Xl, tile_row(r, half) * LDA + cols[u], fmaxf(acc[0][u][r] + bb, 0.f));
        }
        lds_barrier();
    }

    // ---- a = fc_gamma[2](g); softmax over the KNN neighbours; res = sum attn * (v + delta) ----
    f32x16 acc[1][CT];
#pragma unroll
    for (int u = 0; u < CT; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][u][r] = 0.f;
    PTT_STAMP(5);
    gemm_split<D>(Xh, Xl, LDA, p.Wg2s, w, lane, acc, pre);
    PTT_STAMP(6);
    // softmax_j(a_j / sqrt(D)): fc_gamma[2].bias is the same for every neighbour and cancels (never read)
    const float kexp = 1.4426950408889634f / sqrtf((float)D);
    float vv[CT][16];
#pragma unroll
    for (int u = 0; u < CT; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            vv[u][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                rq, nrow[r] + u * 128 * (int)sizeof(float), 2 * D * (int)sizeof(float), 0));
#pragma unroll
    for (int u = 0; u < CT; ++u) {
#pragma unroll
        for (int pp = 0; pp < PTS; ++pp) {
            float s[G];
            float m = acc[0][u][pp * G];
#pragma unroll
            for (int r = 1; r < G; ++r) m = fmaxf(m, acc[0][u][pp * G + r]);
            m = max_halves(m);
            float sum = 0.f, o = 0.f;
#pragma unroll
            for (int r = 0; r < G; ++r) {
                const int rr = pp * G + r;
                s[r] = __builtin_amdgcn_exp2f((acc[0][u][rr] - m) * kexp);
                sum += s[r];
                o += s[r] * (vv[u][rr] + delta[0][u][rr]);
            }
            sum = add_halves(sum);
            o = add_halves(o);
            const float rsum = __builtin_amdgcn_rcpf(sum);
            if (p.attn && pp < npts) {
#pragma unroll
                for (int r = 0; r < G; ++r) {
                    const int row = tile_row(pp * G + r, half);  // = pp*KNN + j
                    p.attn[((size_t)pt[pp] * KNN + (row & (KNN - 1))) * D + cols[u]] = s[r] * rsum;
                }
            }
            if (half == 0 && pp < npts) p.res[(size_t)pt[pp] * D + cols[u]] = o * rsum;
        }
    }
    PTT_STAMP(7);
}

template <int D>
static void (*pair_split_kernel(int k))(AttnSplitParams) {
    return k == 8 ? pt_attn_pair_split_kernel<D, 8> : k == 16 ? pt_attn_pair_split_kernel<D, 16> : pt_attn_pair_split_kernel<D, 32>;
}

}  // namespace ptt

using namespace ptt;

extern "C" int ptt_split_weight_elems(int Cout, int K) {
    if (Cout <= 0 || K <= 0 || (long long)Cout * K > 0x3fffffffLL) return 0;
    return 2 * Cout * K;
}

extern "C" int ptt_pack_weight_split_bf16(const float* W, int Cout, int K, void* out, ptt_stream_t stream) {
    if (Cout <= 0 || K <= 0 || Cout % 32 != 0 || K % 16 != 0 || (long long)Cout * K > 0x3fffffffLL)
        return fail(PTT_EINVAL, "ptt_pack_weight_split_bf16: Cout=%d K=%d (Cout %% 32 == 0 and K %% 16 == 0 are required)", Cout, K);
    if (!W || !out) return fail(PTT_EINVAL, "ptt_pack_weight_split_bf16: null pointer");
    const size_t total = (size_t)2 * Cout * K;
    size_t g = (total + 255) / 256;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(pack_weight_split_kernel, dim3((unsigned)g), dim3(256), 0, as_stream(stream), W, K, Cout / 32, total,
                       static_cast<unsigned short*>(out));
    return check_launch("pack_weight_split_kernel");
}

extern "C" int ptt_pt_attn_pair_split_f32(const ptt_attn_split_desc* d, ptt_stream_t stream) {
    if (!d) return fail(PTT_EINVAL, "ptt_pt_attn_pair_split_f32: null descriptor");
    if (d->B < 0 || d->N <= 0) return fail(PTT_EINVAL, "ptt_pt_attn_pair_split_f32: B=%d N=%d", d->B, d->N);
    if ((d->D != 128 && d->D != 256 && d->D != 512) || (d->k != 8 && d->k != 16 && d->k != 32))
        return fail(PTT_EUNSUPPORTED, "ptt_pt_attn_pair_split_f32: D=%d k=%d (D 128, 256, 512 x k 8, 16, 32 are instantiated)", d->D, d->k);
    if (d->B == 0) return PTT_OK;
    if (!d->xyz || !d->knn || !d->qkv || !d->Wd1p || !d->Wd2s || !d->bd2 || !d->Wg1s || !d->bg1 || !d->Wg2s || !d->res)
        return fail(PTT_EINVAL, "ptt_pt_attn_pair_split_f32: null pointer");
    const int pts = 32 / d->k;                                        // points per 32-row tile
    if (d->N % pts != 0)
        return fail(PTT_EUNSUPPORTED, "ptt_pt_attn_pair_split_f32: N=%d must be a multiple of %d (a tile holds %d points of one cloud)",
                    d->N, pts, pts);
    if (d->N < d->k) return fail(PTT_EUNSUPPORTED, "ptt_pt_attn_pair_split_f32: N=%d < k=%d", d->N, d->k);
    AttnSplitParams p;
    p.xyz = d->xyz; p.rel = d->rel; p.knn = d->knn; p.qkv = d->qkv; p.Wd1p = d->Wd1p; p.Wd2s = d->Wd2s; p.bd2 = d->bd2;
    p.Wg1s = d->Wg1s; p.bg1 = d->bg1; p.Wg2s = d->Wg2s; p.res = d->res; p.attn = d->attn;
    p.order = d->order;
    p.BN = d->B * d->N; p.N = d->N;
    p.first_wave = 512; p.stagger = dev_switches().pair_stagger;
    p.dbg = dev_switches().stamps;
    // two bf16 planes [32][D + 8], the neighbour offsets, the fp32 rel rows
    int lds = 2 * 32 * (d->D + 8) * (int)sizeof(unsigned short) + 32 * (int)sizeof(int) + 32 * 12 * (int)sizeof(float);
    lds += dev_switches().pair_lds_pad;
    const dim3 grid((p.BN + pts - 1) / pts);
    return launch("pt_attn_pair_split_kernel",
                  d->D == 128 ? pair_split_kernel<128>(d->k) : d->D == 256 ? pair_split_kernel<256>(d->k) : pair_split_kernel<512>(d->k),
                  grid, dim3(256), lds, as_stream(stream), p);
}

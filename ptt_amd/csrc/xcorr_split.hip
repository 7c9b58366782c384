// Split-bf16 form of the fused CosineSimAug kernel (gfx950): ptt_xcorr_split_f32, the opt-in arithmetic of
// CosineSimAug.precision = 'bf16x2' on the batched branch (cosine map + xcorr_fused_kernel<2, false> of mfma_ops.hip) at the one
// shape the shipped configuration has: C0 = 256 and two remaining layers, 256 -> 256 (ReLU) -> 256, over all 64-row chunks of
// (template, search) pairs of one search point, max over the template axis.
//
// Arithmetic. h0 = max(P[b,i,:] + w_sim * cos_t[b,j,i], 0) is formed in fp32 by the fp32 kernel's FMA (its folded branch: the
// BatchNorm of layer 0 is already inside P and w_sim). h0 is then written as two bf16 pieces, hi = bf16(x) (round to nearest
// even) and lo = bf16(x - float(hi)); each layer takes per 16-channel K-block three v_mfma_f32_32x32x16_bf16 into ONE fp32
// accumulator, a_hi . w_hi + a_hi . w_lo + a_lo . w_hi. The accumulators start at zero (an inline constant: four splat shift
// vectors would hold 64 registers across the whole chunk loop); layer 1's shift is added and its ReLU taken in fp32 and h1 is
// split again; the max over a chunk's 64 template rows, layer 2's shift (after the max: fp32 rounding is monotonic, so
// max(x) + s = max(x + s) bit for bit), the running max over the chunks, the ReLU after the max (when asked for) and the store
// are fp32.
//
// Geometry: the fp32 kernel's. One four-wave workgroup per search point, 64 template rows per chunk; wave w owns the 32-column
// tiles w and w + 4 over both 32-row tiles (four f32x16 accumulators) in both layers. ONE LDS tile: layer 1 rewrites it in place
// behind a workgroup barrier. The 64 cosines of a chunk are one coalesced load per wave and reach the rows by v_readlane: no
// LDS staging, no barrier for them.
//
// LDS image: two bf16 planes [64][256 + 8]. Lane l reads row l & 31, elements 16 kb + 8 (l >> 5) .. + 7 of a plane with one
// ds_read_b128; the row stride of 132 dwords is 4 mod 8, one 16-byte bank group further per row (the rule pair_split.hip
// documents). 2 planes x 64 x 264 x 2 B = 67 584 B: two workgroups per CU.
//
// Weights: ptt_pack_weight_split_bf16's order (include/ptt_hip.h), fetched two K-blocks ahead with raw buffer loads; the first
// two K-blocks of the NEXT GEMM (layer 2's, or layer 1's of the next chunk) are requested inside the last K-blocks of the
// running one and ride across the epilogue and its barriers.
#include "common.h"
#include "mfma_common.h"

namespace ptt {

typedef __bf16 xbf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 xbf16x4 __attribute__((ext_vector_type(4)));
typedef float xf32x2 __attribute__((ext_vector_type(2)));

constexpr int XSP_LDA = 264;                       // bf16 elements per row of a plane: 256 channels + 8
constexpr int XSP_PLANE = 64 * XSP_LDA;            // bf16 elements per plane
constexpr int XSP_WK = 8 * 2048;                   // bytes per K-block of a split pack with 8 column tiles
constexpr int XSP_WLO = 1024, XSP_WT4 = 4 * 2048;  // the lo piece; column tile w + 4

// mfma_ops.hip's stagger_second_slot, restated (as pair_split.hip and sa_split.hip restate it): the workgroup on a CU's second
// LDS allocation starts `quanta` x ~8k cycles late in the first wave of workgroups (speed only).
__device__ __forceinline__ void xcorr_split_stagger_second_slot(int first_wave_blocks, int quanta) {
    if ((int)blockIdx.x < first_wave_blocks && quanta > 0) {
        const unsigned alloc = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 6);   // HW_REG_LDS_ALLOC
        const unsigned lds_base = alloc & 0xffu, lds_size = (alloc >> 12) & 0x1ffu;
        int slot = lds_size ? (int)(lds_base / lds_size) : 0;
        if (lds_base != 0 && slot == 0) slot = 1;
        for (int i = 0; i < slot * quanta; ++i) __builtin_amdgcn_s_sleep(127);
    }
}

struct XcorrSplitParams {
    const float* cos_t; const float* P; const float* wsim;
    const void* W1s; const float* sh1; const void* W2s; const float* sh2;
    float* out;
    int osb, osc, osn;
    int B, Ns, Nt;
    int relu2;
    int first_wave, stagger;
};

__device__ __forceinline__ xbf16x8 xsp_bf(const f32x4& v) { return __builtin_bit_cast(xbf16x8, v); }

// hi / lo pieces of x at Xh[i] / Xl[i]
__device__ __forceinline__ void xsp_put_split(unsigned short* Xh, unsigned short* Xl, int i, float x) {
    const __bf16 h = (__bf16)x;
    const __bf16 l = (__bf16)(x - (float)h);
    Xh[i] = __builtin_bit_cast(unsigned short, h);
    Xl[i] = __builtin_bit_cast(unsigned short, l);
}

// the first two K-blocks of a 256 -> 256 split pack for column tiles w, w + 4: [kb][2 u + piece]
__device__ __forceinline__ void xsp_prefetch(__amdgpu_buffer_rsrc_t wr, int wvoff, f32x4 (&pre)[2][4]) {
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int i = 0; i < 4; ++i) pre[k][i] = weight_load(wr, wvoff, k * XSP_WK + (i >> 1) * XSP_WT4 + (i & 1) * XSP_WLO);
}

// One 256 -> 256 layer of the 64-row tile at (Ah, Al) (this lane's A fragment inside each plane): column tiles w, w + 4 of the
// pack `wr`, both row tiles, 16 K-blocks of 12 MFMAs into acc (started at zero). `pre`: this pack's first two K-blocks;
// `nxt` <- the first two K-blocks of `wrn`, requested at K-block 14.
__device__ __forceinline__ void xsp_gemm(const unsigned short* Ah, const unsigned short* Al, __amdgpu_buffer_rsrc_t wr, int wvoff,
                                         const f32x4 (&pre)[2][4], f32x16 (&acc)[2][2], __amdgpu_buffer_rsrc_t wrn, f32x4 (&nxt)[2][4]) {
    xbf16x8 ah[2][2], al[2][2];                            // [stage][row tile], A one K-block ahead
    f32x4 b[3][4];                                         // [stage][2 u + piece], weights two K-blocks ahead
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#define XSP_A(S, KB)                                                                               \
    {                                                                                              \
        ah[S][0] = *reinterpret_cast<const xbf16x8*>(Ah + (KB) * 16);                              \
        ah[S][1] = *reinterpret_cast<const xbf16x8*>(Ah + 32 * XSP_LDA + (KB) * 16);               \
        al[S][0] = *reinterpret_cast<const xbf16x8*>(Al + (KB) * 16);                              \
        al[S][1] = *reinterpret_cast<const xbf16x8*>(Al + 32 * XSP_LDA + (KB) * 16);               \
    }
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int i = 0; i < 4; ++i) b[k][i] = pre[k][i];
    XSP_A(0, 0)
#pragma unroll
    for (int kb = 0; kb < 16; ++kb) {
        const int s = kb & 1, sb = kb % 3;
        if (kb < 14) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                b[(kb + 2) % 3][i] = weight_load(wr, wvoff, (kb + 2) * XSP_WK + (i >> 1) * XSP_WT4 + (i & 1) * XSP_WLO);
        } else if (kb == 14) {
            xsp_prefetch(wrn, wvoff, nxt);
        }
        if (kb < 15) XSP_A(s ^ 1, kb + 1)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
                acc[rt][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[s][rt], xsp_bf(b[sb][2 * u]), kb == 0 ? zero16 : acc[rt][u], 0, 0, 0);
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
                acc[rt][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[s][rt], xsp_bf(b[sb][2 * u + 1]), acc[rt][u], 0, 0, 0);
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
                acc[rt][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[s][rt], xsp_bf(b[sb][2 * u]), acc[rt][u], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
#undef XSP_A
}

__global__ __launch_bounds__(256, 2) void xcorr_split_kernel(XcorrSplitParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned short xsp_smem[];
    unsigned short* const Xh = xsp_smem;                   // the chunk's activations (h0, then h1): hi / lo planes
    unsigned short* const Xl = xsp_smem + XSP_PLANE;
    const int t = threadIdx.x, lane = t & 63, half = lane >> 5, col = lane & 31;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int j = logical_block();                         // flat search point b * Ns + jj: a cloud's points share an XCD's L2
    const int b = j / p.Ns, jj = j - b * p.Ns;
    xcorr_split_stagger_second_slot(p.first_wave, p.stagger);
    const __amdgpu_buffer_rsrc_t rP = weight_rsrc(p.P);
    const __amdgpu_buffer_rsrc_t wr1 = weight_rsrc(p.W1s), wr2 = weight_rsrc(p.W2s);
    const int wvoff = (w * 128 + lane) * 16;               // column tile w, piece 0, this lane (bytes)
    f32x4 pre1[2][4], pre2[2][4];
    xsp_prefetch(wr1, wvoff, pre1);
    const f32x4 w4 = *reinterpret_cast<const f32x4*>(p.wsim + lane * 4);   // layer 0: this lane's channel quad, rows w, w + 4, ...
    float sh1[2], sh2[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        sh1[u] = p.sh1 ? p.sh1[(w + 4 * u) * 32 + col] : 0.f;
        sh2[u] = p.sh2 ? p.sh2[(w + 4 * u) * 32 + col] : 0.f;
    }
    const float* cos_row = p.cos_t + (unsigned)(j * p.Nt);
    const int aoff = (lane & 31) * XSP_LDA + 8 * half;     // this lane's A fragment inside a plane (bf16 elements)
    float run[2] = {-__builtin_inff(), -__builtin_inff()};  // running max over the template axis of column tiles w, w + 4

    for (int i0 = 0; i0 < p.Nt; i0 += 64) {
        // ---- layer 0: max(P_i + w_sim * cos_i, 0) in fp32 (the fp32 kernel's packed FMAs), split, -> X ----
        const float cs_l = cos_row[i0 + lane];             // the chunk's 64 cosines, one per lane
        const int prow = (b * p.Nt + i0 + w) * 1024;       // byte offset of row w of the chunk in P
        f32x4 pv[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) pv[k] = weight_load(rP, lane * 16, prow + k * 4096);
        if (i0 != 0) lds_barrier();                        // the previous chunk's layer 2 has read X
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int i = w + 4 * k;
            const float cs = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, cs_l), i));
            const xf32x2 c2 = {cs, cs};
            const xf32x2 lo = __builtin_elementwise_fma(xf32x2{w4[0], w4[1]}, c2, xf32x2{pv[k][0], pv[k][1]});
            const xf32x2 hi = __builtin_elementwise_fma(xf32x2{w4[2], w4[3]}, c2, xf32x2{pv[k][2], pv[k][3]});
            const float y[4] = {fmaxf(lo[0], 0.f), fmaxf(lo[1], 0.f), fmaxf(hi[0], 0.f), fmaxf(hi[1], 0.f)};
            xbf16x4 h, l;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                h[e] = (__bf16)y[e];
                l[e] = (__bf16)(y[e] - (float)h[e]);
            }
            *reinterpret_cast<xbf16x4*>(Xh + i * XSP_LDA + lane * 4) = h;
            *reinterpret_cast<xbf16x4*>(Xl + i * XSP_LDA + lane * 4) = l;
            if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // four rows at a time: bounds the live temporaries
        }
        lds_barrier();                                     // h0 is complete

        // ---- layer 1: 256 -> 256, ReLU, split, back into X ----
        f32x16 acc[2][2];
        xsp_gemm(Xh + aoff, Xl + aoff, wr1, wvoff, pre1, acc, wr2, pre2);
        lds_barrier();                                     // every wave is done with h0
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    xsp_put_split(Xh, Xl, (rt * 32 + tile_row(r, half)) * XSP_LDA + (w + 4 * u) * 32 + col, fmaxf(acc[rt][u][r] + sh1[u], 0.f));
        lds_barrier();                                     // h1 is complete

        // ---- layer 2: 256 -> 256, then the max over this chunk's 64 template rows into the running max ----
        xsp_gemm(Xh + aoff, Xl + aoff, wr2, wvoff, pre2, acc, wr1, pre1);
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
                float m = acc[rt][u][0];
#pragma unroll
                for (int r = 1; r < 16; ++r) m = fmaxf(m, acc[rt][u][r]);
                run[u] = fmaxf(run[u], max_halves(m) + sh2[u]);     // max(x) + s = max(x + s): rounding is monotonic
            }
    }
    if (half == 0) {
        float* o = p.out + (b * p.osb + jj * p.osn);
#pragma unroll
        for (int u = 0; u < 2; ++u) o[((w + 4 * u) * 32 + col) * p.osc] = p.relu2 ? fmaxf(run[u], 0.f) : run[u];
    }
}

}  // namespace ptt

using namespace ptt;

extern "C" int ptt_xcorr_split_f32(const ptt_xcorr_split_desc* d, ptt_stream_t stream) {
    if (!d) return fail(PTT_EINVAL, "ptt_xcorr_split_f32: null descriptor");
    if (d->B < 0 || d->Ns < 0) return fail(PTT_EINVAL, "ptt_xcorr_split_f32: B=%d Ns=%d", d->B, d->Ns);
    if (d->B == 0 || d->Ns == 0) return PTT_OK;
    if (!d->cos_t || !d->P || !d->w_sim || !d->W1s || !d->W2s || !d->out) return fail(PTT_EINVAL, "ptt_xcorr_split_f32: null pointer");
    if ((reinterpret_cast<uintptr_t>(d->P) & 15) != 0 || (reinterpret_cast<uintptr_t>(d->w_sim) & 15) != 0 ||
        (reinterpret_cast<uintptr_t>(d->W1s) & 15) != 0 || (reinterpret_cast<uintptr_t>(d->W2s) & 15) != 0)
        return fail(PTT_EINVAL, "ptt_xcorr_split_f32: P, w_sim, W1s and W2s must be 16-byte aligned");
    if (d->out_sb < 0 || d->out_sc < 0 || d->out_sn < 0) return fail(PTT_EINVAL, "ptt_xcorr_split_f32: negative output stride");
    if (d->Nt <= 0 || (d->Nt % 64) != 0)
        return fail(PTT_EUNSUPPORTED, "ptt_xcorr_split_f32: Nt=%d (the template seeds are walked in chunks of 64)", d->Nt);
    {   // 32-bit byte offsets (buffer descriptors, scalar index arithmetic)
        const unsigned long long lim = 0x7fffffffull, B = (unsigned long long)d->B;
        const unsigned long long out_last = (B - 1) * (unsigned long long)d->out_sb + (unsigned long long)(d->Ns - 1) * (unsigned long long)d->out_sn +
                                            255ull * (unsigned long long)d->out_sc;
        if (B * d->Ns * d->Nt * 4ull >= lim || B * d->Nt * 256ull * 4ull >= lim || out_last * 4ull >= lim)
            return fail(PTT_EUNSUPPORTED, "ptt_xcorr_split_f32: B=%d Ns=%d Nt=%d: an array of this launch exceeds 2 GiB "
                        "(32-bit offsets) — split the batch", d->B, d->Ns, d->Nt);
    }
    XcorrSplitParams p;
    p.cos_t = d->cos_t; p.P = d->P; p.wsim = d->w_sim;
    p.W1s = d->W1s; p.sh1 = d->shift1; p.W2s = d->W2s; p.sh2 = d->shift2; p.out = d->out;
    p.osb = (int)d->out_sb; p.osc = (int)d->out_sc; p.osn = (int)d->out_sn;
    p.B = d->B; p.Ns = d->Ns; p.Nt = d->Nt;
    p.relu2 = d->relu2 ? 1 : 0;
    p.first_wave = 1024; p.stagger = 2;                    // as ptt_xcorr_fused_fwd_f32
    const int lds = 2 * XSP_PLANE * (int)sizeof(unsigned short);
    return launch("xcorr_split_kernel", xcorr_split_kernel, dim3(d->B * d->Ns), dim3(256), lds, as_stream(stream), p);
}

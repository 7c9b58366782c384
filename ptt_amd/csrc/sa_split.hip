// Split-bf16 form of the streamed set-abstraction kernel (gfx950): ptt_sa_stream_split_f32, the opt-in arithmetic of
// PointnetSAModuleVotes.precision = 'bf16x2' on the dense SA1 / SA2 levels (hoisted 128-channel layer 0, then
// 128 -> 128 -> 256, 32 neighbours) — the one shape sa_stream_kernel<32> (mfma_ops.hip) serves, and no other.
//
// Arithmetic. h0 = act(term[idx] + Wx . rel) is formed in fp32 exactly as the fp32 kernel forms it (the normalize_xyz divide,
// three FMAs in the same order, the l0_relu floor). h0 is then written as two bf16 pieces, hi = bf16(x) (round to nearest
// even) and lo = bf16(x - float(hi)); layers 1 and 2 take per 16-channel K-block three v_mfma_f32_32x32x16_bf16 into ONE fp32
// accumulator, a_hi . w_hi + a_hi . w_lo + a_lo . w_hi. Layer 1's fp32 shift is the C operand of its first MFMA, its ReLU runs
// in fp32 and h1 is split again; layer 2's shift, its ReLU (when asked for) and the max over the 32 neighbours run on the fp32
// accumulators, and the store is fp32.
//
// Geometry: the fp32 kernel's. A persistent workgroup walks `chunk` consecutive 64-row tiles of two centres each (rows
// 16 w .. 16 w + 15 are wave w's: centre w >> 1 of the tile, neighbours 16 (w & 1) ..). Two LDS tiles: P (h0, gathered by every
// wave for tile n + 1 inside its own layer-2 MFMA stream of tile n, one row pair per K-block) and Q (h1). The max-pool of tile
// n's accumulators and the index -> coordinates -> meta chain of tile n + 1 sit inside layer 1's stream.
//
// LDS image: a tile is two bf16 planes [64][128 + 8]. Lane l reads row l & 31, elements 16 kb + 8 (l >> 5) .. + 7 of a plane
// with one ds_read_b128; the row stride of 68 dwords is 4 mod 8, one 16-byte bank group further per row (the rule
// pair_split.hip documents). 2 tiles x 2 planes x 64 x 136 x 2 B = 69 632 B + 1 KiB of meta rows: two workgroups per CU.
//
// Weights: ptt_pack_weight_split_bf16's order (include/ptt_hip.h), fetched two K-blocks ahead with raw buffer loads.
#include <math.h>
#include "common.h"
#include "mfma_common.h"

namespace ptt {

typedef __bf16 sbf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 sbf16x4 __attribute__((ext_vector_type(4)));

constexpr int SSP_LDA = 136;                       // bf16 elements per row of a plane: 128 channels + 8
constexpr int SSP_PLANE = 64 * SSP_LDA;            // bf16 elements per plane

// mfma_ops.hip's stagger_second_slot, restated (as pair_split.hip restates it): the workgroup on a CU's second LDS
// allocation starts `quanta` x ~8k cycles late in the first wave of workgroups (speed only).
__device__ __forceinline__ void sa_split_stagger_second_slot(int first_wave_blocks, int quanta) {
    if ((int)blockIdx.x < first_wave_blocks && quanta > 0) {
        const unsigned alloc = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 6);   // HW_REG_LDS_ALLOC
        const unsigned lds_base = alloc & 0xffu, lds_size = (alloc >> 12) & 0x1ffu;
        int slot = lds_size ? (int)(lds_base / lds_size) : 0;
        if (lds_base != 0 && slot == 0) slot = 1;
        for (int i = 0; i < slot * quanta; ++i) __builtin_amdgcn_s_sleep(127);
    }
}

struct SaSplitParams {
    const float* xyz; const float* new_xyz; const int32_t* idx;
    const float* term; const float* wx;
    const void* W1s; const float* sh1; const void* W2s; const float* sh2;
    float* out;
    int osb, osc, osm;
    int B, N, M;
    int tiles, chunk;
    int l0_relu, relu2, normalize;
    float radius;
    int first_wave, stagger;
};

// a centre index with its (cloud, index inside the cloud), advanced without divisions (mfma_ops.hip's SasCentre)
struct SspCentre {
    int c, b, m;
    __device__ __forceinline__ void advance(int k, int M) {
        c += k; m += k;
        while (m >= M) { m -= M; ++b; }
    }
};

// h0 of one row pair (rows 2i, 2i+1 of the wave's 16 -> lanes 0-31 / 32-63, four channels per lane): the fp32 kernel's FMA
// chain (sas_pair_store), then the split, one ds_write_b64 per plane
__device__ __forceinline__ void ssp_pair_store(unsigned short* Xh, unsigned short* Xl, int w, int i, int sub, int q, f32x4 v,
                                               const f32x4& m, const f32x4& wx0, const f32x4& wx1, const f32x4& wx2, float floor) {
    sbf16x4 h, l;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float y = __builtin_fmaf(wx0[j], m[1], v[j]);
        y = __builtin_fmaf(wx1[j], m[2], y);
        y = __builtin_fmaf(wx2[j], m[3], y);
        y = fmaxf(y, floor);
        h[j] = (__bf16)y;
        l[j] = (__bf16)(y - (float)h[j]);
    }
    const int e = (16 * w + 2 * i + sub) * SSP_LDA + q * 4;
    *reinterpret_cast<sbf16x4*>(Xh + e) = h;
    *reinterpret_cast<sbf16x4*>(Xl + e) = l;
}

// hi / lo pieces of x at Xh[i] / Xl[i]
__device__ __forceinline__ void ssp_put_split(unsigned short* Xh, unsigned short* Xl, int i, float x) {
    const __bf16 h = (__bf16)x;
    const __bf16 l = (__bf16)(x - (float)h);
    Xh[i] = __builtin_bit_cast(unsigned short, h);
    Xl[i] = __builtin_bit_cast(unsigned short, l);
}

// max over the 32 neighbour rows of one 32 x 32 accumulator tile, + shift, ReLU: sas_pool of the fp32 kernel
__device__ __forceinline__ float ssp_pool(const f32x16& a, float sh, int relu) {
    float mx = a[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, a[r]);
    mx = max_halves(mx) + sh;
    return relu ? fmaxf(mx, 0.f) : mx;
}

__device__ __forceinline__ sbf16x8 ssp_bf(const f32x4& v) { return __builtin_bit_cast(sbf16x8, v); }

__global__ __launch_bounds__(256, 2) void sa_stream_split_kernel(SaSplitParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned short ssp_smem[];
    unsigned short* const Ph = ssp_smem;                       // h0 of the current tile, hi / lo planes
    unsigned short* const Pl = ssp_smem + SSP_PLANE;
    unsigned short* const Qh = ssp_smem + 2 * SSP_PLANE;       // h1 of the current tile
    unsigned short* const Ql = ssp_smem + 3 * SSP_PLANE;
    float* const meta = reinterpret_cast<float*>(ssp_smem + 4 * SSP_PLANE);   // [4 waves][16 rows][off, dx, dy, dz]
    const int t = threadIdx.x, lane = t & 63, half = lane >> 5, sub = half, q = lane & 31;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int tile0 = logical_block() * p.chunk;
    const int ntiles = min(p.chunk, p.tiles - tile0);
    if (ntiles <= 0) return;
    sa_split_stagger_second_slot(p.first_wave, p.stagger);
    const __amdgpu_buffer_rsrc_t rf = weight_rsrc(p.term);
    const __amdgpu_buffer_rsrc_t wr1 = weight_rsrc(p.W1s), wr2 = weight_rsrc(p.W2s);
    const int wvoff = (w * 128 + lane) * 16;               // column tile w, piece 0, this lane (bytes)
    constexpr int WK1 = 4 * 2048, WK2 = 8 * 2048;          // bytes per K-block of a split pack (NT = 4 / 8)
    constexpr int WLO = 1024, WT4 = 4 * 2048;              // the lo piece; column tile w + 4
    const f32x4 wx0 = *reinterpret_cast<const f32x4*>(p.wx + q * 4);
    const f32x4 wx1 = *reinterpret_cast<const f32x4*>(p.wx + 128 + q * 4);
    const f32x4 wx2 = *reinterpret_cast<const f32x4*>(p.wx + 256 + q * 4);
    const int col = lane & 31;
    const float sh1 = p.sh1 ? p.sh1[w * 32 + col] : 0.f;
    const float sh2a = p.sh2 ? p.sh2[w * 32 + col] : 0.f;
    const float sh2b = p.sh2 ? p.sh2[(w + 4) * 32 + col] : 0.f;
    f32x16 sh1v;                                           // layer 1's shift as the C operand of its first MFMAs
#pragma unroll
    for (int r = 0; r < 16; ++r) sh1v[r] = sh1;
    const int total_centres = p.B * p.M;
    const float floor0 = p.l0_relu ? 0.f : -__builtin_inff();
    const float rdiv = p.normalize ? p.radius : 1.0f;      // x / 1 is exact: one code path
    const int M = p.M, N = p.N;
    const int osb = p.osb, osm = p.osm;
    const int ocol0 = (w * 32 + col) * p.osc, ocol1 = ((w + 4) * 32 + col) * p.osc;

    SspCentre own, first;                                  // the wave's own centre of a tile; the tile's first centre
    {
        const int c0 = tile0 * 2;
        first.c = c0; first.b = c0 / M; first.m = c0 - first.b * M;
        own = first;
        own.advance(w >> 1, M);
    }
    // index -> (relative coordinates, byte offset of the neighbour's term row) of the wave's 16 rows, all 64 lanes
    // redundantly (lane & 15): no exec-mask change inside an MFMA stream
    auto meta_index = [&](const SspCentre& ce) -> int {
        const int c = ce.c < total_centres ? ce.c : total_centres - 1;
        return p.idx[(size_t)c * 32 + 16 * (w & 1) + (lane & 15)];
    };
    struct MetaXyz { float x, y, z, cx, cy, cz; int flat; };
    auto meta_fetch = [&](const SspCentre& ce, int n) -> MetaXyz {
        const bool in = ce.c < total_centres;
        const int c = in ? ce.c : total_centres - 1;
        const int b = in ? ce.b : p.B - 1;
        MetaXyz r;
        r.flat = b * N + n;
        r.x = p.xyz[(size_t)r.flat * 3 + 0]; r.y = p.xyz[(size_t)r.flat * 3 + 1]; r.z = p.xyz[(size_t)r.flat * 3 + 2];
        r.cx = p.new_xyz[(size_t)c * 3 + 0]; r.cy = p.new_xyz[(size_t)c * 3 + 1]; r.cz = p.new_xyz[(size_t)c * 3 + 2];
        return r;
    };
    auto meta_store = [&](const MetaXyz& r) {
        const float dx = (r.x - r.cx) / rdiv, dy = (r.y - r.cy) / rdiv, dz = (r.z - r.cz) / rdiv;
        const int off = r.flat * (128 * (int)sizeof(float));
        *reinterpret_cast<f32x4*>(meta + (w * 16 + (lane & 15)) * 4) = f32x4{__builtin_bit_cast(float, off), dx, dy, dz};
    };

    // ---- prologue: the first tile is gathered in the open ----
    f32x4 pre1[2][2];                                      // layer 1's first two K-blocks: [kb][piece]
#pragma unroll
    for (int k = 0; k < 2; ++k) { pre1[k][0] = weight_load(wr1, wvoff, k * WK1); pre1[k][1] = weight_load(wr1, wvoff, k * WK1 + WLO); }
    {
        const int n = meta_index(own);
        meta_store(meta_fetch(own, n));
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const f32x4 m = *reinterpret_cast<const f32x4*>(meta + (w * 16 + 2 * i + sub) * 4);
            const f32x4 v = weight_load(rf, __builtin_bit_cast(int, m[0]) + q * 16, 0);
            ssp_pair_store(Ph, Pl, w, i, sub, q, v, m, wx0, wx1, wx2, floor0);
        }
    }

    f32x16 acc[2][2];                                      // layer 2's accumulators [row tile][column tile]: pooled inside the NEXT tile's layer 1
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[rt][u][r] = 0.f;
    float pv[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
    SspCentre prev = first;                                // first centre of the tile whose accumulators are pending
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    auto store_pooled = [&](const SspCentre& f) {          // the two centres of a tile: scalar index arithmetic
        SspCentre c1 = f;
        c1.advance(1, M);
        if (half == 0) {
            if (f.c < total_centres) {
                float* o = p.out + (f.b * osb + f.m * osm);
                o[ocol0] = pv[0][0]; o[ocol1] = pv[0][1];
            }
            if (c1.c < total_centres) {
                float* o = p.out + (c1.b * osb + c1.m * osm);
                o[ocol0] = pv[1][0]; o[ocol1] = pv[1][1];
            }
        }
    };

    const int aoff = (lane & 31) * SSP_LDA + 8 * half;     // this lane's A fragment inside a plane (bf16 elements)

    for (int it = 0; it < ntiles; ++it) {
        const bool more = it + 1 < ntiles;                 // last tile: re-gathers itself (branch-free loop)
        SspCentre own_next = own;
        if (more) own_next.advance(2, M);
        lds_barrier();                                     // A: P is complete; every wave is done with Q
        const int nn = meta_index(own_next);               // index load in flight under the first K-blocks
        MetaXyz mx;

        // ---- layer 1: 128 -> 128, column tile w, both row tiles; inside its MFMA stream the max-pool of the PREVIOUS tile's
        // layer-2 accumulators and the (index -> coordinates -> meta) chain of the NEXT tile ----
        f32x16 acc1[2];
        {
            const unsigned short* ah_p = Ph + aoff;
            const unsigned short* al_p = Pl + aoff;
            sbf16x8 ah[2][2], al[2][2];                    // [stage][row tile], A one K-block ahead
            f32x4 b[3][2];                                 // [stage][piece], weights two K-blocks ahead
#define SSP_A(S, HP, LP, KB)                                                                       \
            {                                                                                      \
                ah[S][0] = *reinterpret_cast<const sbf16x8*>(HP + (KB) * 16);                      \
                ah[S][1] = *reinterpret_cast<const sbf16x8*>(HP + 32 * SSP_LDA + (KB) * 16);       \
                al[S][0] = *reinterpret_cast<const sbf16x8*>(LP + (KB) * 16);                      \
                al[S][1] = *reinterpret_cast<const sbf16x8*>(LP + 32 * SSP_LDA + (KB) * 16);       \
            }
            b[0][0] = pre1[0][0]; b[0][1] = pre1[0][1]; b[1][0] = pre1[1][0]; b[1][1] = pre1[1][1];
            SSP_A(0, ah_p, al_p, 0)
#pragma unroll
            for (int kb = 0; kb < 8; ++kb) {
                const int s = kb & 1, sb = kb % 3;
                if (kb < 6) {
                    b[(kb + 2) % 3][0] = weight_load(wr1, wvoff, (kb + 2) * WK1);
                    b[(kb + 2) % 3][1] = weight_load(wr1, wvoff, (kb + 2) * WK1 + WLO);
                }
                if (kb < 7) SSP_A(s ^ 1, ah_p, al_p, kb + 1)
                if (kb == 4) mx = meta_fetch(own_next, nn);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
                    acc1[rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[s][rt], ssp_bf(b[sb][0]), kb == 0 ? sh1v : acc1[rt], 0, 0, 0);
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
                    acc1[rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[s][rt], ssp_bf(b[sb][1]), acc1[rt], 0, 0, 0);
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
                    acc1[rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[s][rt], ssp_bf(b[sb][0]), acc1[rt], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (kb < 4) pv[kb >> 1][kb & 1] = ssp_pool(acc[kb >> 1][kb & 1], (kb & 1) ? sh2b : sh2a, p.relu2);
                if (kb == 6) meta_store(mx);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        f32x4 pre2[2][4];                                  // layer 2's first two K-blocks ride across the epilogue: [kb][2 u + piece]
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int i = 0; i < 4; ++i) pre2[k][i] = weight_load(wr2, wvoff, k * WK2 + (i >> 1) * WT4 + (i & 1) * WLO);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                ssp_put_split(Qh, Ql, (rt * 32 + tile_row(r, half)) * SSP_LDA + w * 32 + col, fmaxf(acc1[rt][r], 0.f));
        if (it > 0) store_pooled(prev);
        lds_barrier();                                     // C: h1 is complete; every wave is done with P

        // ---- layer 2: 128 -> 256 (column tiles w, w + 4), with the gather of the next tile inside the MFMA stream ----
        {
            const unsigned short* ah_p = Qh + aoff;
            const unsigned short* al_p = Ql + aoff;
            sbf16x8 ah[2][2], al[2][2];
            f32x4 b[3][4];                                 // [stage][2 u + piece]
#pragma unroll
            for (int k = 0; k < 2; ++k)
#pragma unroll
                for (int i = 0; i < 4; ++i) b[k][i] = pre2[k][i];
            SSP_A(0, ah_p, al_p, 0)
            // (row offset, rel) of row pair kb is read one iteration ahead: the term load that depends on it must not put an
            // LDS round trip in front of the iteration's MFMAs
            f32x4 mc = *reinterpret_cast<const f32x4*>(meta + (w * 16 + sub) * 4), mn = mc;
#pragma unroll
            for (int kb = 0; kb < 8; ++kb) {               // K-block kb and row pair kb of the next tile
                const int s = kb & 1, sb = kb % 3;
                if (kb < 6) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        b[(kb + 2) % 3][i] = weight_load(wr2, wvoff, (kb + 2) * WK2 + (i >> 1) * WT4 + (i & 1) * WLO);
                } else if (kb == 6) {                      // the next tile's first layer-1 weights
#pragma unroll
                    for (int k = 0; k < 2; ++k) { pre1[k][0] = weight_load(wr1, wvoff, k * WK1); pre1[k][1] = weight_load(wr1, wvoff, k * WK1 + WLO); }
                }
                if (kb < 7) {
                    SSP_A(s ^ 1, ah_p, al_p, kb + 1)
                    mn = *reinterpret_cast<const f32x4*>(meta + (w * 16 + 2 * (kb + 1) + sub) * 4);
                }
                const f32x4 v = weight_load(rf, __builtin_bit_cast(int, mc[0]) + q * 16, 0);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int rt = 0; rt < 2; ++rt)
                        acc[rt][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[s][rt], ssp_bf(b[sb][2 * u]), kb == 0 ? zero16 : acc[rt][u], 0, 0, 0);
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int rt = 0; rt < 2; ++rt)
                        acc[rt][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[s][rt], ssp_bf(b[sb][2 * u + 1]), acc[rt][u], 0, 0, 0);
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int rt = 0; rt < 2; ++rt)
                        acc[rt][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[s][rt], ssp_bf(b[sb][2 * u]), acc[rt][u], 0, 0, 0);
                ssp_pair_store(Ph, Pl, w, kb, sub, q, v, mc, wx0, wx1, wx2, floor0);
                __builtin_amdgcn_sched_barrier(0);
                mc = mn;
            }
#undef SSP_A
        }
        prev = first;
        if (more) { first.advance(2, M); own = own_next; }
    }
    // ---- the last tile's max over the 32 neighbours, one centre per row tile ----
#pragma unroll
    for (int i = 0; i < 4; ++i) pv[i >> 1][i & 1] = ssp_pool(acc[i >> 1][i & 1], (i & 1) ? sh2b : sh2a, p.relu2);
    store_pooled(prev);
}

}  // namespace ptt

using namespace ptt;

extern "C" int ptt_sa_stream_split_f32(const ptt_sa_split_desc* d, ptt_stream_t stream) {
    if (!d) return fail(PTT_EINVAL, "ptt_sa_stream_split_f32: null descriptor");
    if (d->B < 0 || d->N <= 0 || d->M < 0) return fail(PTT_EINVAL, "ptt_sa_stream_split_f32: B=%d N=%d M=%d", d->B, d->N, d->M);
    if (d->B == 0 || d->M == 0) return PTT_OK;
    if (!d->xyz || !d->new_xyz || !d->idx || !d->l0_point_term || !d->l0_xyz_weight || !d->W1s || !d->W2s || !d->out)
        return fail(PTT_EINVAL, "ptt_sa_stream_split_f32: null pointer");
    if ((reinterpret_cast<uintptr_t>(d->l0_point_term) & 15) != 0 || (reinterpret_cast<uintptr_t>(d->l0_xyz_weight) & 15) != 0 ||
        (reinterpret_cast<uintptr_t>(d->W1s) & 15) != 0 || (reinterpret_cast<uintptr_t>(d->W2s) & 15) != 0)
        return fail(PTT_EINVAL, "ptt_sa_stream_split_f32: l0_point_term, l0_xyz_weight, W1s and W2s must be 16-byte aligned");
    if (d->out_sb < 0 || d->out_sc < 0 || d->out_sm < 0)
        return fail(PTT_EINVAL, "ptt_sa_stream_split_f32: negative output stride");
    {   // 32-bit byte offsets (buffer descriptors, scalar index arithmetic), as in ptt_sa_fused_fwd_f32
        const unsigned long long lim = 0x7fffffffull, B = (unsigned long long)d->B;
        const unsigned long long out_last = (B - 1) * (unsigned long long)d->out_sb + (unsigned long long)(d->M - 1) * (unsigned long long)d->out_sm +
                                            255ull * (unsigned long long)d->out_sc;
        if (B * d->N * 12ull >= lim || B * d->M * 32ull * 4ull >= lim || B * d->M * 256ull * 4ull >= lim || B * d->N * 128ull * 4ull >= lim ||
            out_last * 4ull >= lim)
            return fail(PTT_EUNSUPPORTED, "ptt_sa_stream_split_f32: B=%d N=%d M=%d: an array of this launch exceeds 2 GiB "
                        "(32-bit offsets) — split the batch", d->B, d->N, d->M);
    }
    SaSplitParams p;
    p.xyz = d->xyz; p.new_xyz = d->new_xyz; p.idx = d->idx; p.term = d->l0_point_term; p.wx = d->l0_xyz_weight;
    p.W1s = d->W1s; p.sh1 = d->shift1; p.W2s = d->W2s; p.sh2 = d->shift2; p.out = d->out;
    p.osb = (int)d->out_sb; p.osc = (int)d->out_sc; p.osm = (int)d->out_sm;
    p.B = d->B; p.N = d->N; p.M = d->M;
    p.l0_relu = d->l0_relu ? 1 : 0; p.relu2 = d->relu2 ? 1 : 0; p.normalize = d->normalize_xyz ? 1 : 0; p.radius = d->radius;
    p.first_wave = 1024; p.stagger = dev_switches().sa_stagger;
    // the tile walk of sa_stream_kernel<32>: 64-row tiles of two centres, at most 512 resident workgroups, short chunks
    const int total_centres = d->B * d->M;
    p.tiles = (total_centres + 1) / 2;
    int wgs = p.tiles < 512 ? p.tiles : 512;
    p.chunk = (p.tiles + wgs - 1) / wgs;
    if (dev_switches().sa_chunk > 0 && p.chunk > dev_switches().sa_chunk) p.chunk = dev_switches().sa_chunk;
    wgs = (p.tiles + p.chunk - 1) / p.chunk;
    const int lds = 4 * SSP_PLANE * (int)sizeof(unsigned short) + 4 * 16 * 4 * (int)sizeof(float);
    return launch("sa_stream_split_kernel", sa_stream_split_kernel, dim3(wgs), dim3(256), lds, as_stream(stream), p);
}

// Body of the Point-Transformer pair kernels (mfma_ops.hip: pt_attn_pair_kernel<D>, pt_attn_pair_heads_kernel<HEADS>),
// included inside both kernel definitions with D, HEADS and `AttnParams p` in scope. Written out in each kernel instead of
// called as an inlined device function: the single-head kernel then compiles to exactly the instructions it had before
// the multi-head form existed (an inlined body is optimised before it meets the kernel's attributes and comes out
// differently scheduled). Not a header to include anywhere else.
    constexpr int KNN = 16, NT = D / 32, CT = NT / 4, LDK = D + 4, NKB = D / 8;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Xs = smem;                                       // [32][LDK]
    int* nb = reinterpret_cast<int*>(smem + 32 * LDK);      // [32] flat neighbour row (b*N + n)
    constexpr int LDR = 12;                                 // [rel.x rel.y rel.z 1 | 0 0 0 0] + pad (stride = 4 mod 8)
    float* relt = smem + 32 * LDK + 32;                     // [32][LDR]: the A operand of fc_delta[0]
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, half = lane >> 5;
    const int slot0 = logical_block() * 2;                   // the tile's two point slots
    const int npts = min(2, p.BN - slot0);
    // the points behind the slots (ptt_spatial_order_f32: neighbours in space next to each other in launch order); both lie in
    // the same cloud (N is even, the order permutes inside clouds)
    const int s0 = slot0 < p.BN ? slot0 : p.BN - 1, s1 = slot0 + 1 < p.BN ? slot0 + 1 : p.BN - 1;
    const int pt0 = p.order ? p.order[s0] : s0, pt1 = p.order ? p.order[s1] : s1;
    f32x4 pre[CT];
    prefetch_first_block_full<CT>(p.Wd1p, w, lane, pre);    // fc_delta[0]'s only weight block: requested first
    stagger_second_slot(p.first_wave, p.stagger);
    PTT_STAMP(0);

    if (t < 32) {
        const int pt = (t >> 4) ? pt1 : pt0;
        const int b = pt / p.N;
        const int n = p.knn[(size_t)pt * KNN + (t & 15)];
        const int flat = b * p.N + n;
        nb[t] = n * (3 * D * (int)sizeof(float));      // byte offset of the neighbour's q|k|v row inside its cloud
        f32x4 r4;
        if (p.rel) {                                   // precomputed by the kNN kernel: no index -> xyz dependency
            const float* rl = p.rel + ((size_t)pt * KNN + (t & 15)) * 3;
            r4 = f32x4{rl[0], rl[1], rl[2], 1.f};
        } else {
            r4 = f32x4{p.xyz[(size_t)pt * 3 + 0] - p.xyz[(size_t)flat * 3 + 0],
                       p.xyz[(size_t)pt * 3 + 1] - p.xyz[(size_t)flat * 3 + 1],
                       p.xyz[(size_t)pt * 3 + 2] - p.xyz[(size_t)flat * 3 + 2], 1.f};
        }
        *reinterpret_cast<f32x4*>(relt + t * LDR) = r4;
        *reinterpret_cast<f32x4*>(relt + t * LDR + 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    lds_barrier();

    int cols[CT];
#pragma unroll
    for (int u = 0; u < CT; ++u) cols[u] = (w + 4 * u) * 32 + (lane & 31);

    // fc_delta[0] + ReLU: h = relu([rel 1] . [W | b]^T) as ONE K-block of MFMAs (K = 4, zero-padded to 8) instead of
    // ~500 vector-ALU instructions per wave — next to the other workgroup's MFMA stream those crawl (DESIGN.md lesson 8)
    {
        f32x16 h[1][CT];
        zero_acc(h);
        gemm_core<1, CT, CT, 4, 1>(relt, LDR, 1, reinterpret_cast<const f32x4*>(p.Wd1p), NT, w, lane, h, pre);
        prefetch_first_block_full<CT>(p.Wd2p, w, lane, pre);    // fc_delta[2]'s first weight block
#pragma unroll
        for (int u = 0; u < CT; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) Xs[tile_row(r, half) * LDK + cols[u]] = fmaxf(h[0][u][r], 0.f);
    }
    lds_barrier();

    PTT_STAMP(1);
    // ---- delta = fc_delta[2](h) ----
    f32x16 delta[1][CT];
    zero_acc(delta);
    gemm_core<1, CT, CT, 4, PTT_PAIR_PF>(Xs, LDK, NKB, reinterpret_cast<const f32x4*>(p.Wd2p), NT, w, lane, delta, pre);
    if constexpr (HEADS == 1) prefetch_first_block_full<CT>(p.Wg1p, w, lane, pre);    // next GEMM's first block: in flight across the epilogue
    else prefetch_first_block_heads<D, HEADS>(p.Wg1p, w, lane, pre);
#pragma unroll
    for (int u = 0; u < CT; ++u) {
        const float bb = p.bd2[cols[u]];
#pragma unroll
        for (int r = 0; r < 16; ++r) delta[0][u][r] += bb;
    }
    PTT_STAMP(2);
    // Gathers of neighbour k / v rows: raw buffer loads on a descriptor based at the cloud's first q|k|v row. The
    // per-(row, lane) byte offset is ONE 32-bit VGPR per tile row; channel group and the k / v column block are
    // immediates or an SGPR — a flat 64-bit address per load costs 3-4 vector-ALU instructions, 64 loads per phase.
    const int cloud = pt0 / p.N;
    const __amdgpu_buffer_rsrc_t rq = weight_rsrc(p.qkv + (size_t)cloud * p.N * 3 * D);
    int nrow[16];  // byte offset of (neighbour row, this lane's first column) for each of this lane's 16 tile rows
#pragma unroll
    for (int r = 0; r < 16; ++r) nrow[r] = nb[tile_row(r, half)] + (w * 32 + (lane & 31)) * (int)sizeof(float);

    lds_barrier();  // all waves done with h
    // t = (q_i - k_j) + delta  -> X
    {
        const int pa = pt0, pb = (npts > 1) ? pt1 : pt0;
#pragma unroll
        for (int u = 0; u < CT; ++u) {
            const float qa = p.qkv[(size_t)pa * 3 * D + cols[u]];
            const float qb = p.qkv[(size_t)pb * 3 * D + cols[u]];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float kv = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                    rq, nrow[r] + (D + u * 128) * (int)sizeof(float), 0, 0));
                const float q = (r < 8) ? qa : qb;
                Xs[tile_row(r, half) * LDK + cols[u]] = (q - kv) + delta[0][u][r];
            }
        }
    }
    lds_barrier();

    PTT_STAMP(3);
    // ---- g = relu(fc_gamma[0](t)) -> X ----
    {
        f32x16 acc[1][CT];
        zero_acc(acc);
        if constexpr (HEADS == 1) {
            gemm_core<1, CT, CT, 4, PTT_PAIR_PF>(Xs, LDK, NKB, reinterpret_cast<const f32x4*>(p.Wg1p), NT, w, lane, acc, pre);
            prefetch_first_block_full<CT>(p.Wg2p, w, lane, pre);
        } else {
            gemm_heads<D, HEADS>(Xs, LDK, p.Wg1p, w, lane, acc, pre);
            prefetch_first_block_heads<D, HEADS>(p.Wg2p, w, lane, pre);
        }
        PTT_STAMP(4);
        lds_barrier();
#pragma unroll
        for (int u = 0; u < CT; ++u) {
            const float bb = p.bg1[cols[u]];
#pragma unroll
            for (int r = 0; r < 16; ++r) Xs[tile_row(r, half) * LDK + cols[u]] = fmaxf(acc[0][u][r] + bb, 0.f);
        }
        lds_barrier();
    }

    // ---- a = fc_gamma[2](g); softmax over the 16 neighbours; res = sum attn * (v + delta) ----
    f32x16 acc[1][CT];
    zero_acc(acc);
    PTT_STAMP(5);
    if constexpr (HEADS == 1)
        gemm_core<1, CT, CT, 4, PTT_PAIR_PF>(Xs, LDK, NKB, reinterpret_cast<const f32x4*>(p.Wg2p), NT, w, lane, acc, pre);
    else
        gemm_heads<D, HEADS>(Xs, LDK, p.Wg2p, w, lane, acc, pre);
    PTT_STAMP(6);
    // softmax_j((a_j + b) / sqrt(D)) over the 16 neighbours of a point: the bias b is the same for every neighbour, so
    // it cancels (fc_gamma[2].bias is never read); 1/sqrt(D) and log2(e) are one constant inside exp2; the weighted sum
    // is normalised once at the end. Fewer vector-ALU instructions next to the other workgroup's MFMA stream.
    const float kexp = 1.4426950408889634f / sqrtf((float)(D / HEADS));     // multi-head: 1 / sqrt(hd)
    // all 64 neighbour values of this lane are requested before any softmax arithmetic: one L2 round trip
    // instead of eight (the gathers, not the math, were the length of this phase)
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
        for (int pp = 0; pp < 2; ++pp) {
            float s[8];
            float m = acc[0][u][pp * 8];
#pragma unroll
            for (int r = 1; r < 8; ++r) m = fmaxf(m, acc[0][u][pp * 8 + r]);
            m = max_halves(m);
            float sum = 0.f, o = 0.f;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int rr = pp * 8 + r;
                s[r] = __builtin_amdgcn_exp2f((acc[0][u][rr] - m) * kexp);
                sum += s[r];
                o += s[r] * (vv[u][rr] + delta[0][u][rr]);
            }
            sum = add_halves(sum);
            o = add_halves(o);
            const float rsum = __builtin_amdgcn_rcpf(sum);
            if (p.attn && pp < npts) {
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const int row = tile_row(pp * 8 + r, half);  // = pp*16 + j
                    if constexpr (HEADS == 1) {
                        p.attn[((size_t)(pp ? pt1 : pt0) * KNN + (row & 15)) * D + cols[u]] = s[r] * rsum;
                    } else {                                     // the reference's (B*heads, N, k, hd) layout
                        constexpr int HD = D / HEADS;
                        const int pt = pp ? pt1 : pt0, b = pt / p.N, n = pt - b * p.N;
                        p.attn[((((size_t)b * HEADS + cols[u] / HD) * p.N + n) * KNN + (row & 15)) * HD + cols[u] % HD] =
                            s[r] * rsum;
                    }
                }
            }
            if (half == 0 && pp < npts) p.res[(size_t)(pp ? pt1 : pt0) * D + cols[u]] = o * rsum;
        }
    }
    PTT_STAMP(7);

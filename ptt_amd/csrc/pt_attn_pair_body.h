// Body of the Point-Transformer pair kernels (mfma_ops.hip: pt_attn_pair_kernel<D, KNN>, pt_attn_pair_heads_kernel<D, KNN, HEADS>),
// included inside both kernel definitions with D, KNN, HEADS and `AttnParams p` in scope. Written out in each kernel instead of
// called as an inlined device function: the single-head kernel then compiles to exactly the instructions it had before
// the multi-head form existed (an inlined body is optimised before it meets the kernel's attributes and comes out
// differently scheduled). Not a header to include anywhere else.
// A 32-row tile holds PTS = 32 / KNN whole points (4 / 2 / 1 at 8 / 16 / 32 neighbours). With tile_row(r, half) =
// (r & 3) + 8 (r >> 2) + 4 half, accumulator register r of EVERY lane belongs to point r / G, G = KNN / 2, and each point's
// rows lie half in each half-wave: the softmax is PTS groups of G registers closed by one max_halves / add_halves.
    static_assert(KNN == 8 || KNN == 16 || KNN == 32, "a 32-row tile splits into whole points");
    static_assert(D % 128 == 0, "4 waves x 32 columns per column-tile round");
    constexpr int NT = D / 32, CT = NT / 4, LDK = D + 4, NKB = D / 8;
    constexpr int PTS = 32 / KNN, G = KNN / 2;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Xs = smem;                                       // [32][LDK]
    int* nb = reinterpret_cast<int*>(smem + 32 * LDK);      // [32] flat neighbour row (b*N + n)
    constexpr int LDR = 12;                                 // [rel.x rel.y rel.z 1 | 0 0 0 0] + pad (stride = 4 mod 8)
    float* relt = smem + 32 * LDK + 32;                     // [32][LDR]: the A operand of fc_delta[0]
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, half = lane >> 5;
    const int slot0 = logical_block() * PTS;                 // the tile's PTS point slots
    const int npts = min(PTS, p.BN - slot0);
    // the points behind the slots (ptt_spatial_order_f32: neighbours in space next to each other in launch order); all lie in
    // the same cloud (N % PTS == 0, the order permutes inside clouds)
    // (scalars chosen by constant conditions, not arrays filled in loops: at KNN = 16 this is, token for token, what the kernel
    //  was compiled from before KNN became a parameter — an array form comes out differently scheduled)
#define PTT_SLOT(i) (slot0 + (i) < p.BN ? slot0 + (i) : p.BN - 1)
    const int s0 = slot0 < p.BN ? slot0 : p.BN - 1, s1 = PTS > 1 ? PTT_SLOT(1) : s0;
    const int s2 = PTS > 2 ? PTT_SLOT(2) : s0, s3 = PTS > 2 ? PTT_SLOT(3) : s0;
#undef PTT_SLOT
    const int pt0 = p.order ? p.order[s0] : s0, pt1 = PTS > 1 ? (p.order ? p.order[s1] : s1) : pt0;
    const int pt2 = PTS > 2 ? (p.order ? p.order[s2] : s2) : pt0, pt3 = PTS > 2 ? (p.order ? p.order[s3] : s3) : pt0;
    const int pt[4] = {pt0, pt1, pt2, pt3};                 // indexed by unrolled loop counters only
    f32x4 pre[CT];
    prefetch_first_block_full<CT>(p.Wd1p, w, lane, pre);    // fc_delta[0]'s only weight block: requested first
    stagger_second_slot(p.first_wave, p.stagger);
    PTT_STAMP(0);

    if (t < 32) {
        // row t: point t / KNN of the tile, neighbour t % KNN
        const int me = PTS == 1 ? pt0 : PTS == 2 ? ((t >> 4) ? pt1 : pt0) : ((t >> 4) ? ((t & 8) ? pt3 : pt2) : ((t & 8) ? pt1 : pt0));
        const int b = me / p.N;
        const int n = p.knn[(size_t)me * KNN + (t & (KNN - 1))];
        const int flat = b * p.N + n;
        nb[t] = n * (3 * D * (int)sizeof(float));      // byte offset of the neighbour's q|k|v row inside its cloud
        f32x4 r4;
        if (p.rel) {                                   // precomputed by the kNN kernel: no index -> xyz dependency
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
    const int cloud = pt[0] / p.N;
    const __amdgpu_buffer_rsrc_t rq = weight_rsrc(p.qkv + (size_t)cloud * p.N * 3 * D);
    int nrow[16];  // byte offset of (neighbour row, this lane's first column) for each of this lane's 16 tile rows
#pragma unroll
    for (int r = 0; r < 16; ++r) nrow[r] = nb[tile_row(r, half)] + (w * 32 + (lane & 31)) * (int)sizeof(float);

    lds_barrier();  // all waves done with h
    // t = (q_i - k_j) + delta  -> X
    {
        // a slot past the last point reads the tile's first point
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

    // ---- a = fc_gamma[2](g); softmax over the KNN neighbours; res = sum attn * (v + delta) ----
    f32x16 acc[1][CT];
    zero_acc(acc);
    PTT_STAMP(5);
    if constexpr (HEADS == 1)
        gemm_core<1, CT, CT, 4, PTT_PAIR_PF>(Xs, LDK, NKB, reinterpret_cast<const f32x4*>(p.Wg2p), NT, w, lane, acc, pre);
    else
        gemm_heads<D, HEADS>(Xs, LDK, p.Wg2p, w, lane, acc, pre);
    PTT_STAMP(6);
    // softmax_j((a_j + b) / sqrt(D)) over the KNN neighbours of a point: the bias b is the same for every neighbour, so
    // it cancels (fc_gamma[2].bias is never read); 1/sqrt(D) and log2(e) are one constant inside exp2; the weighted sum
    // is normalised once at the end. Fewer vector-ALU instructions next to the other workgroup's MFMA stream.
    const float kexp = 1.4426950408889634f / sqrtf((float)(D / HEADS));     // multi-head: 1 / sqrt(hd)
    // all 16 CT neighbour values of this lane are requested before any softmax arithmetic: one L2 round trip
    // instead of 2 CT (the gathers, not the math, were the length of this phase)
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
                    if constexpr (HEADS == 1) {
                        p.attn[((size_t)pt[pp] * KNN + (row & (KNN - 1))) * D + cols[u]] = s[r] * rsum;
                    } else {                                     // the reference's (B*heads, N, k, hd) layout
                        constexpr int HD = D / HEADS;
                        const int b = pt[pp] / p.N, n = pt[pp] - b * p.N;
                        p.attn[((((size_t)b * HEADS + cols[u] / HD) * p.N + n) * KNN + (row & (KNN - 1))) * HD + cols[u] % HD] =
                            s[r] * rsum;
                    }
                }
            }
            if (half == 0 && pp < npts) p.res[(size_t)pt[pp] * D + cols[u]] = o * rsum;
        }
    }
    PTT_STAMP(7);

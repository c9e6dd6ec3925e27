// vb_attn_stream_body.inc -- the body of vbs::attn_stream_kernel<L> and vbs::attn_stream_masked_kernel<L> (vb_attn_stream.h), written once
// and included into both: the including kernel provides its parameters (qk, vt, out, heads), `constexpr bool MASKED` and
// `const uint32_t* bits` (the key bitmap; unused when !MASKED).  Text inclusion, not a shared __device__ function: with the body
// behind a call the compiler allocates attn_stream_kernel<720> 170 VGPRs for 168 and its occupancy falls from 3 to 2 waves per SIMD; this
// way the unmasked kernels compile exactly as they did before the masked ones existed.
    constexpr int HD = 64, KS = HD / 32, DT = HD / 16;
    constexpr int NT = L / 16;                         // query tiles
    constexpr int NSUB = (L + 31) / 32;                // 32-key sub-chunks, the last one partial when L % 32 != 0
    constexpr int NCH = (NSUB + 1) / 2;                // chunks
    constexpr int LAST_SUB = NSUB - 2 * (NCH - 1);     // sub-chunks of the last chunk (1 or 2)
    constexpr bool PARTIAL = L % 32 != 0;
    constexpr int SPLITS = splits<L>();
    static_assert(L % 16 == 0 && L % 8 == 0 && NCH >= 2, "token count");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fh = blockIdx.x / SPLITS, sp = blockIdx.x - fh * SPLITS;
    const int f = fh / heads, h = fh - f * heads, C = heads * HD;
    const bf16* qf = qk + (size_t)f * L * 2 * C + h * HD;          // q rows of this frame / head
    const bf16* kf = qf + C;
    const bf16* vf = vt + ((size_t)f * C + h * HD) * L;
    const int l15 = lane & 15, q = lane >> 4;
    const uint32_t* fb = MASKED ? bits + (size_t)f * NSUB : nullptr;      // this frame's words: one per 32-key sub-chunk

    // this wave's query tiles; a slot past the last tile recomputes the last tile and stores nothing
    int qts[NQ];
    bf16x8 qfrag[NQ][KS];
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
        qts[u] = sp * QT_PER_WG + w * NQ + u;
        const int qt = qts[u] < NT ? qts[u] : NT - 1;
        vba::load_q(qfrag[u], qf, qt, l15, q, C);
    }

    // ---- staging: chunk c's K rows (permuted) and V^T columns into buffer `b`, nsub 32-key sub-chunks of it; 2 nsub pieces per wave
    const int pl = vbg::swz_byte(lane * 16), prow = pl >> 6, pk = (pl & 63) >> 1;
    auto stage = [&](int c, int b, int nsub) {
        char* Kimg = smem + b * CHUNK_BYTES;
        char* Vimg = Kimg + KC * HD * 2;
        for (int s = w; s < nsub * 2 * KS; s += WAVES) {           // K sub-tile s = key tile t (of this chunk) x k-step
            const int t = s / KS, ks = s - t * KS;
            vbg::glds16(kf + (size_t)(c * KC + vba::perm_key(t, prow)) * 2 * C + ks * 32 + pk, Kimg + s * 1024 + lane * 16);
        }
        for (int s = w; s < nsub * DT; s += WAVES) {               // V^T sub-tile s = d tile x sub-chunk (sub-chunk fastest)
            const int dt = s / nsub, sc = s - dt * nsub;
            vbg::glds16(vf + (size_t)(dt * 16 + prow) * L + c * KC + sc * 32 + pk, Vimg + (dt * 2 + sc) * 1024 + lane * 16);
        }
    };

    const int fr = vbg::swz_byte(l15 * 64 + q * 16);
    float mrun[NQ], lsum[NQ];
    f4 O[NQ][DT];
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
        mrun[u] = -1e30f;
        lsum[u] = 0.f;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) O[u][dt] = splat4(0.f);
    }

    // ---- one chunk: S^T = K q^T on NS sub-chunks, online softmax, O^T += V^T P^T
    auto compute = [&](auto ns_tag, auto mask_tag, int c, int b) {
        constexpr int NS = decltype(ns_tag)::value;
        constexpr bool MASK = decltype(mask_tag)::value;
        const char* Kimg = smem + b * CHUNK_BYTES;
        const char* Vimg = Kimg + KC * HD * 2;
        f4 S[NQ][2 * NS];
        vba::qk_tiles(S, Kimg, fr, qfrag);
        if constexpr (MASKED) {    // every sub-chunk: the lane's byte of the sub-chunk's word, bits 0-3 the even tile's keys, 4-7 the odd tile's
#pragma unroll
            for (int sc = 0; sc < NS; ++sc) {
                const uint32_t kb = fb[2 * c + sc] >> (8 * q);
#pragma unroll
                for (int u = 0; u < NQ; ++u)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (!((kb >> j) & 1u)) S[u][2 * sc][j] = -INFINITY;
                        if (!((kb >> (4 + j)) & 1u)) S[u][2 * sc + 1][j] = -INFINITY;
                    }
            }
        } else if constexpr (MASK) {      // the last sub-chunk: this lane's keys are base + {0..3} (even tile) and base + 4 + {0..3} (odd tile)
            const int base = c * KC + (NS - 1) * 32 + 8 * q;
#pragma unroll
            for (int u = 0; u < NQ; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (base + j >= L) S[u][2 * NS - 2][j] = -INFINITY;
                    if (base + 4 + j >= L) S[u][2 * NS - 1][j] = -INFINITY;
                }
        }
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
            const float mx = fmaxf(mrun[u], quad_max(vba::lane_max(S[u])));      // finite: every chunk holds an existing key (MASKED: chunk 0 does, and m never falls)
            const float alpha = __builtin_amdgcn_exp2f((mrun[u] - mx) * vba::LOG2E);
            mrun[u] = mx;
            // vba::exp_rows(S[u], mx), its loop written out: with the loop inside a helper attn_stream_kernel<320> takes 168 VGPRs for 166
            const vbg::f2 l2 = {vba::LOG2E, vba::LOG2E}, nmb = {-mx * vba::LOG2E, -mx * vba::LOG2E};
            vbg::f2 s0 = {0.f, 0.f}, s1 = {0.f, 0.f};
#pragma unroll
            for (int t = 0; t < 2 * NS; ++t) vba::exp_tile(S[u][t], l2, nmb, s0, s1);
            const vbg::f2 st = s0 + s1;
            lsum[u] = fmaf(lsum[u], alpha, st.x + st.y);      // this lane's keys only: the four lane groups are summed once, at the end
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) O[u][dt] = O[u][dt] * splat4(alpha);
        }
#pragma unroll
        for (int sc = 0; sc < NS; ++sc) {
            if constexpr (MASKED) {      // this lane's V^T columns are the same eight keys: the absent ones are 0
                const uint32_t kb = fb[2 * c + sc] >> (8 * q);
                vba::pv_chunk(O, S, sc, Vimg, 2, fr, [&](bf16x8& vf8) {
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (!((kb >> j) & 1u)) vf8[j] = (bf16)0.0f;
                });
            } else if (MASK && sc == NS - 1) {      // this lane's V^T columns are keys base + {0..7}: those past the frame are not the frame's, so they are 0
                const int base = c * KC + sc * 32 + 8 * q;
                vba::pv_chunk(O, S, sc, Vimg, 2, fr, [&](bf16x8& vf8) {
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (base + j >= L) vf8[j] = (bf16)0.0f;
                });
            } else vba::pv_chunk(O, S, sc, Vimg, 2, fr);
        }
    };

    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    stage(0, 0, 2);
    for (int c = 0; c + 1 < NCH; ++c) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's pieces of chunk c (and, at c = 0, its q fragments)
        __syncthreads();                                     // chunk c is whole; nobody reads chunk c - 1's buffer any more
        stage(c + 1, (c + 1) & 1, c + 2 < NCH ? 2 : LAST_SUB);
        compute(I2{}, std::false_type{}, c, c & 1);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if constexpr (LAST_SUB == 2) compute(I2{}, std::integral_constant<bool, PARTIAL>{}, NCH - 1, (NCH - 1) & 1);
    else compute(I1{}, std::integral_constant<bool, PARTIAL>{}, NCH - 1, (NCH - 1) & 1);

#pragma unroll
    for (int u = 0; u < NQ; ++u) {
        const float inv = 1.0f / quad_sum(lsum[u]);
        if (qts[u] < NT) vba::store_tile(out, (size_t)(f * L + qts[u] * 16 + l15), C, h * HD + q * 4, O[u], inv);
    }

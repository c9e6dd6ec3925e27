// vb_attn_stream.h -- key-streaming multi-head self-attention for token counts that fit neither the LDS nor one softmax row in
// registers (OSTrack-384: L = 144 + 576 = 720), bf16 MFMA, gfx950.  Same arithmetic as vb_attn.h (v_mfma_f32_16x16x32_bf16, keys on
// the MFMA rows for S^T = K q^T, P rounded to bf16 and fed to O^T = V^T P^T from S^T's own registers, f32 max / sum / accumulators,
// exp2 with the log2 e factor), same inputs and output: qk [M][2 C] (q pre-scaled | k) from the EPI_BF16 GEMM, vt [frame][C][L] from
// the EPI_VT GEMM, out [M][C].
//
// Plan.  One workgroup = one (frame, head, query range): 4 waves x NQ = 3 query tiles of 16 = 192 queries, all of a wave's tiles in ONE
// pass over the keys, so a (frame, head) is split over ceil(L / 192) workgroups (L = 720: 4, the last with 9 of its 12 tile slots in
// use; L = 320: 2).  Keys are streamed in chunks of KC = 64 (L = 720: 11 whole chunks + one of 32 keys of which 16 exist; L = 320: 5
// whole chunks) with an online softmax: per query a running max m and a per-lane partial sum l; when a chunk moves the max, l and
// the O accumulators are rescaled by exp2((m_old - m_new) log2 e).  m starts at -1e30 (finite: no inf - inf), so the first chunk's
// rescale factor is exactly 0 on accumulators that are exactly 0.
//
// LDS: a chunk is 8 KiB of K (4 key tiles x 2 k-steps of 1 KiB st_16x32 sub-tiles, rows permuted as in vb_attn.h so that P's
// B-operand is S^T's registers) + 8 KiB of V^T (4 d tiles x 2 32-key sub-chunks) = 16 KiB, double-buffered: 32 KiB per workgroup
// (<= 80 KiB: two workgroups per CU, 8 waves = 2 per SIMD, 256 VGPRs each).  Every piece is one LDS-DMA wave-instruction (vbg::glds16),
// 4 per wave and chunk.  Per chunk ONE barrier: wait for the own pieces of chunk c, barrier (chunk c has landed for everyone, and
// everyone is done reading chunk c - 1's buffer), issue chunk c + 1's DMA into that buffer, then run chunk c's 16 NQ MFMAs per wave
// under it.
//
// Registers per wave (NQ = 3): S 3 x 16 + O 3 x 16 + q fragments 3 x 8 + m, l 6 + K / V^T fragment and P operands + addresses:
// measured 168 VGPRs at L = 720 and 166 at L = 320 of the 256 the two-workgroup occupancy allows, ScratchSize 0
// (profiles/r6_resource_usage.txt).  Every K / V^T fragment read from LDS feeds NQ = 3 MFMAs.
//
// The partial last chunk (L % 32 = 16).  A lane's eight scores of a 32-key sub-chunk are keys 32 c + 8 (lane >> 4) + {0..7}: those
// >= L are set to -inf BEFORE the chunk maximum, so their P is exp2(-inf) = 0 whatever the K rows read there held, and the V^T
// fragment's columns for those keys are set to 0 in registers (the same lane arithmetic: V^T's k elements of a lane are the same eight
// keys), so 0 x V^T is 0 whatever was staged -- a NaN in a neighbour frame cannot reach this one.  What is READ past a frame's last token
// is therefore never used, it only has to be mapped memory: the next frame's rows / the head of the next feature row (possibly stale,
// possibly being written by another chain's GEMM at that moment: whole bf16 elements, discarded either way), and past the last frame
// the 32-row / 32-element tail both workspaces carry (vitb.hip zero-fills them once, at create).
//
// Two kernels share the body below: attn_stream_kernel<L> (every key of the frame) and attn_stream_masked_kernel<L> (a per-frame key
// bitmap: the blocks behind a candidate-elimination stage, vb_ce.h).  They are separate instantiations: the unmasked one carries no
// trace of the bitmap.
//
// Remainder query tiles (45 tiles over 4 x 12 slots): a slot beyond the last tile computes the last tile again and does not store;
// no wave leaves the chunk loop early, every wave meets every barrier.
#pragma once
#include "vb_attn.h"

namespace vbs {

using vbg::bf16;
using vbg::bf16x4;
using vbg::bf16x8;

constexpr int KC = 64;                      // keys per chunk
constexpr int NQ = 3;                       // query tiles per wave
constexpr int WAVES = 4;
constexpr int QT_PER_WG = WAVES * NQ;       // 12 tiles = 192 queries per workgroup
constexpr int CHUNK_BYTES = 2 * KC * 64 * 2;      // K + V^T, HD = 64
constexpr int LDS_BYTES = 2 * CHUNK_BYTES;        // double-buffered: 32 KiB
constexpr int PAD_TOKENS = 32;              // rows (qk) / elements (vt) the last chunk may read past the workspace's last frame

template <int L> constexpr int splits() { return (L / 16 + QT_PER_WG - 1) / QT_PER_WG; }

// The body (vb_attn_stream_body.inc) is written once for the two kernels below.  MASKED: `bits` is the per-frame key bitmap of candidate elimination (vb_ce.h),
// [frame][ceil(L / 32)] uint32, bit set = key present.  A lane's eight keys of 32-key sub-chunk s of the frame are one byte of word s, the
// same for the whole workgroup: byte (lane >> 4), its low four bits the even key tile's scores, its high four the odd tile's.  Absent keys
// get -inf before the chunk maximum and their V^T columns are zeroed in registers, exactly as the partial last chunk does it above and for
// the same reason: nothing a removed row holds can reach a kept one.  The bitmap's bits at and past L are 0, so it covers the partial chunk
// too.  Chunk 0 holds template keys only, which are never removed: the running maximum is finite from the first chunk on, and a later
// chunk that is wholly absent leaves m, l and O as they are (alpha = exp2(0) = 1, P = exp2(-inf) = 0).
// grid = B * heads * splits<L>(), 256 threads, LDS_BYTES of dynamic LDS
template <int L>
__global__ __launch_bounds__(256, 2) void attn_stream_kernel(const bf16* __restrict__ qk, const bf16* __restrict__ vt,
                                                          bf16* __restrict__ out, int heads) {
    constexpr bool MASKED = false;
    const uint32_t* const bits = nullptr;
#include "vb_attn_stream_body.inc"
}

// the same under a key bitmap (candidate elimination, vb_ce.h): bits [frame][ceil(L / 32)]
template <int L>
__global__ __launch_bounds__(256, 2) void attn_stream_masked_kernel(const bf16* __restrict__ qk, const bf16* __restrict__ vt,
                                                                 bf16* __restrict__ out, int heads, const uint32_t* __restrict__ bits) {
    constexpr bool MASKED = true;
#include "vb_attn_stream_body.inc"
}

// The same arithmetic at a RUN-TIME frame length: the compact form of candidate elimination (vb_ce.h), where the kept tokens of a frame
// are gathered into Lp = round_up(nkeys, 16) rows behind each stage.  Lp: rows of a frame in qk / out and the row length of vt, a multiple
// of 16, at least 80 (two chunks); nkeys in (Lp - 16, Lp]: the live rows.  Rows [nkeys, Lp) are pad rows: as keys they get the partial
// last chunk's treatment (-inf before the chunk maximum, V^T columns zeroed in registers) under a plain count -- they all lie in the
// last 16-key tile, so only the last sub-chunk is touched, as in attn_stream_kernel<720> -- and as queries they compute something finite
// that nobody reads.  The last chunk holds one or two sub-chunks (Lp % 32 is 0 or 16); chunk and split counts are run-time values, the
// chunk loop is the one above.  Written out rather than sharing vb_attn_stream_body.inc: the body's token counts are constant expressions,
// and attn_stream_kernel<L> / attn_stream_masked_kernel<L> must go on compiling exactly as recorded (profiles/r6_resource_usage.txt).
// What is read past a frame's last row (Lp % 32 = 16: 16 rows / elements) is never used, as above, and is mapped memory: where Lp < L the
// dense layout leaves it inside the slice's own rows (Lp <= L - 16); where nothing shorter than the full frame results (L = 720 with 561 to
// 575 kept tokens: Lp = 720) it is the next frame's rows, the next chain's slice or the workspaces' tails -- exactly attn_stream_kernel<720>'s reads.
inline int splits_rt(int Lp) { return (Lp / 16 + QT_PER_WG - 1) / QT_PER_WG; }

// grid = B * heads * splits_rt(Lp), 256 threads, LDS_BYTES of dynamic LDS
__global__ __launch_bounds__(256, 2) void attn_stream_rt_kernel(const bf16* __restrict__ qk, const bf16* __restrict__ vt, bf16* __restrict__ out,
                                                             int heads, int Lp, int nkeys) {
    constexpr int HD = 64, KS = HD / 32, DT = HD / 16;
    const int NT = Lp / 16, NSUB = (Lp + 31) / 32, NCH = (NSUB + 1) / 2, LAST_SUB = NSUB - 2 * (NCH - 1);
    const int SPLITS = (NT + QT_PER_WG - 1) / QT_PER_WG;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fh = blockIdx.x / SPLITS, sp = blockIdx.x - fh * SPLITS;
    const int f = fh / heads, h = fh - f * heads, C = heads * HD;
    const bf16* qf = qk + (size_t)f * Lp * 2 * C + h * HD;
    const bf16* kf = qf + C;
    const bf16* vf = vt + ((size_t)f * C + h * HD) * Lp;
    const int l15 = lane & 15, q = lane >> 4;

    int qts[NQ];
    bf16x8 qfrag[NQ][KS];
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
        qts[u] = sp * QT_PER_WG + w * NQ + u;
        const int qt = qts[u] < NT ? qts[u] : NT - 1;
        vba::load_q(qfrag[u], qf, qt, l15, q, C);
    }

    const int pl = vbg::swz_byte(lane * 16), prow = pl >> 6, pk = (pl & 63) >> 1;
    auto stage = [&](int c, int b, int nsub) {
        char* Kimg = smem + b * CHUNK_BYTES;
        char* Vimg = Kimg + KC * HD * 2;
        for (int s = w; s < nsub * 2 * KS; s += WAVES) {
            const int t = s / KS, ks = s - t * KS;
            vbg::glds16(kf + (size_t)(c * KC + vba::perm_key(t, prow)) * 2 * C + ks * 32 + pk, Kimg + s * 1024 + lane * 16);
        }
        for (int s = w; s < nsub * DT; s += WAVES) {
            const int dt = s / nsub, sc = s - dt * nsub;
            vbg::glds16(vf + (size_t)(dt * 16 + prow) * Lp + c * KC + sc * 32 + pk, Vimg + (dt * 2 + sc) * 1024 + lane * 16);
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

    // one chunk, as in the body: MASK = the chunk's last sub-chunk may hold keys at or past nkeys
    auto compute = [&](auto ns_tag, auto mask_tag, int c, int b) {
        constexpr int NS = decltype(ns_tag)::value;
        constexpr bool MASK = decltype(mask_tag)::value;
        const char* Kimg = smem + b * CHUNK_BYTES;
        const char* Vimg = Kimg + KC * HD * 2;
        f4 S[NQ][2 * NS];
        vba::qk_tiles(S, Kimg, fr, qfrag);
        const int base = c * KC + (NS - 1) * 32 + 8 * q;      // this lane's keys of the last sub-chunk: base + {0..7}
        if constexpr (MASK) {
#pragma unroll
            for (int u = 0; u < NQ; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (base + j >= nkeys) S[u][2 * NS - 2][j] = -INFINITY;
                    if (base + 4 + j >= nkeys) S[u][2 * NS - 1][j] = -INFINITY;
                }
        }
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
            const float mx = fmaxf(mrun[u], quad_max(vba::lane_max(S[u])));      // finite: chunk 0 is whole (nkeys > 64)
            const float alpha = __builtin_amdgcn_exp2f((mrun[u] - mx) * vba::LOG2E);
            mrun[u] = mx;
            const vbg::f2 l2 = {vba::LOG2E, vba::LOG2E}, nmb = {-mx * vba::LOG2E, -mx * vba::LOG2E};
            vbg::f2 s0 = {0.f, 0.f}, s1 = {0.f, 0.f};
#pragma unroll
            for (int t = 0; t < 2 * NS; ++t) vba::exp_tile(S[u][t], l2, nmb, s0, s1);
            const vbg::f2 st = s0 + s1;
            lsum[u] = fmaf(lsum[u], alpha, st.x + st.y);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) O[u][dt] = O[u][dt] * splat4(alpha);
        }
#pragma unroll
        for (int sc = 0; sc < NS; ++sc) {
            if (MASK && sc == NS - 1) {
                vba::pv_chunk(O, S, sc, Vimg, 2, fr, [&](bf16x8& vf8) {
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (base + j >= nkeys) vf8[j] = (bf16)0.0f;
                });
            } else vba::pv_chunk(O, S, sc, Vimg, 2, fr);
        }
    };

    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    stage(0, 0, 2);
    for (int c = 0; c + 1 < NCH; ++c) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        stage(c + 1, (c + 1) & 1, c + 2 < NCH ? 2 : LAST_SUB);
        compute(I2{}, std::false_type{}, c, c & 1);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // The last chunk is always the masked instantiation, also where none of its keys is absent (nkeys = Lp, Lp % 32 = 0: a few compares per
    // lane that change nothing).  Branching to unmasked instantiations there was tried: with four instantiations of the chunk behind
    // uniform branches the kernel takes 256 VGPRs and spills 4 of them (20 B scratch) where this form takes 188 and none.
    if (LAST_SUB == 2) compute(I2{}, std::true_type{}, NCH - 1, (NCH - 1) & 1);
    else compute(I1{}, std::true_type{}, NCH - 1, (NCH - 1) & 1);

#pragma unroll
    for (int u = 0; u < NQ; ++u) {
        const float inv = 1.0f / quad_sum(lsum[u]);
        if (qts[u] < NT) vba::store_tile(out, (size_t)(f * Lp + qts[u] * 16 + l15), C, h * HD + q * 4, O[u], inv);
    }
}

}  // namespace vbs

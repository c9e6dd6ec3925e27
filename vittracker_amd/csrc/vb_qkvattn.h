// vb_qkvattn.h -- the qkv projection FUSED into the attention of one (frame, head), bf16 MFMA, gfx950 (round 5).
//
// lib/models/ostrack/vit.py:51-66 (Attention.forward) with norm1 folded in (vb_gemm.h): per frame and head
//     [q | k | v] = rstd * (x W'^T) + b'      x: the frame's L = 320 raw residual rows (bf16), W': the head's 3 x 64 folded weight rows
//     out         = softmax(q k^T) v          (q pre-scaled by 64^-0.5 at load time)
// The separate kernels (qk GEMM, v GEMM, attention) write q / k / v^T for all heads to HBM (378 MB at B = 256) and read them back
// (378 MB): 1.49 GB of fabric traffic per block with their operand re-fetches, in a step whose phases are memory-system-bound
// (NOTES R5-2).  Here one workgroup computes the 320 x 192 projection of ITS (frame, head) into registers, writes q, K and V^T as the
// attention's operand images into LDS and attends on chip: what reaches the fabric is x (the 12 heads of a frame run on one XCD at
// about the same time: one fetch + L2 hits), the head's 295 KB of weights (L2-resident), and the 40 KB output.
//
// Projection: the GEMM of vb_gemm.h at a 320 x 192 tile -- the same 64 KiB of operands per 64-deep k-tile as the 256 x 256 tile
// (X 40 pieces + W 24 pieces of 8 rows x 128 B, chunk ^ row swizzle, LDS-DMA), 8 waves as 4 (token groups of 5 tiles) x 2 (feature
// groups of 6 tiles: q0-1 k0-1 v0-1 | q2-3 k2-3 v2-3), 30 accumulator tiles per wave.  The v tiles swap the MFMA operands (tokens as
// rows), so a lane holds four consecutive TOKENS of one feature: V^T is written transposed, as the P.V product wants it.  Every wave
// has the same tile pattern (which tiles swap is a compile-time property of the tile index): with a wave-uniform branch between two
// operand orders hipcc spilled 300 registers around the k-loop.
// Attention: vb_attn.h's arithmetic (S^T = K q^T with keys on the MFMA rows, softmax rows in registers, O^T = V^T P^T, two query tiles
// per pass) through vb_attn.h's helpers -- nothing of it is written here --, on 8 waves, q from LDS like K; the epilogue places the K
// rows by vba::perm_tile / perm_row, the inverse of the staging kernels' vba::perm_key.  The three images alias the projection's
// staging buffers.
#pragma once
#include "vb_attn.h"

#ifndef VB_QA_DBG
#define VB_QA_DBG 0         // timing experiments only (wrong results): 1 = projection + epilogue only (no attention), 2 = attention only (no k-loop),
                            // 3 / 4 / 5 = mode 1 with every W / X / W and X piece fetched from k-tile 0 of head 0 / frame 0 (L2 hits: what the fill costs),
                            // 6 = mode 1 without the DMAs (stale LDS), 7 = mode 1 without fragment reads and MFMAs (the fill alone)
#endif

namespace vbq {

using vbg::bf16;
using vbg::bf16x4;
using vbg::bf16x8;
using vbg::glds16;
using vbg::swz_byte;

constexpr int L = 320, HD = 64, NT = L / 16, NC = L / 32, KS = HD / 32, DT = HD / 16;
constexpr int XP = L / 8, WP = 3 * HD / 8;                  // 1 KiB DMA pieces per k-tile: 40 + 24
constexpr int STAGE_BYTES = (XP + WP) * 1024;               // 64 KiB
constexpr int IMG_BYTES = NT * KS * 1024;                   // q, K, V^T images: 40 KiB each
constexpr int LDS_BYTES = 2 * STAGE_BYTES;
static_assert(3 * IMG_BYTES <= LDS_BYTES && (XP + WP) % 8 == 0, "images alias the stages; pieces divide over 8 waves");

struct Args {
    const bf16* X;        // [B L][DM] raw residual rows (bf16 copy written by the residual-writing GEMMs)
    const bf16* W;        // [3 DM][DM] folded qkv weights (q rows pre-scaled)
    const float* bias;    // [3 DM]
    const float* rstd;    // [B L] or null
    bf16* out;            // [B L][DM] attention output (head h at columns h HD ..)
    int B, heads;
    int hgroup;           // heads walked together (see the item order in the kernel); divides heads
};

// The kernel's body at model width DM (768: ViT-Base, 1024: ViT-Large, 384: ViT-Small, 192: ViT-Tiny).  DM sets the row pitch of X / W / out, the distance between the q, k
// and v sections of W and bias, and the number of k-tiles (DM / 64); the stages and the images hold 64-deep k-tiles of one head and do not
// depend on it.
template <int DM>
__device__ __forceinline__ void qkv_attn_body(const Args& a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane_k = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = w >> 1, wn = w & 1;
    char* const Qimg = smem;
    char* const Kimg = smem + IMG_BYTES;
    char* const Vimg = smem + 2 * IMG_BYTES;

    // ---- items: XCD x (blocks with blockIdx % 8 == x share an L2) owns frames x, x + 8, ...; its workgroups walk (frame, head) pairs
    // frame-major inside a GROUP of a.hgroup heads, group after group: the heads of a frame run at about the same time on one XCD and
    // share the fetch of its rows, and a group's weight rows (hgroup x 288 KiB) stay nearer than a whole qkv matrix (3.4 MiB against the
    // 4 MiB L2 the frames stream through).  Measured at 256 frames: groups of 12 / 6 / 4 / 3 / 2 / 1 heads 379.9 / 372.5 / 375.4 / 374.7 /
    // 383.0 / 459.2 us per launch -- the order hardly matters until every CU of an XCD reads different rows (VB_QA_HGROUP, default 6)
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, per = gridDim.x >> 3;
    const int nfx = (a.B - xcd + 7) / 8;                     // frames of this XCD
    const int nitems = nfx * a.heads;

    // ---- DMA sources of this wave's 8 pieces per k-tile (piece p = w + 8 i: i < 5 X rows p 8 .., i >= 5 the W rows (w 8 ..) of q / k / v):
    // every piece reads row (w 8 + lane / 8) of ITS 64-row block at the lane's swizzled k offset, so ONE per-lane byte offset serves all
    // eight; what differs per piece is wave-uniform and goes into the scalar base
    const unsigned soff = (unsigned)((w * 8 + (lane_k >> 3)) * DM + (((lane_k & 7) ^ (lane_k >> 3)) * 8)) * 2u;

    for (int li = slot; li < nitems; li += per) {
        const int gsz = nfx * a.hgroup, hg = li / gsz, rem = li - hg * gsz, lf = rem / a.hgroup, h = hg * a.hgroup + rem - lf * a.hgroup, f = xcd + 8 * lf;
        // Every per-lane address of an item comes from a FRESH opaque copy of the lane index: as invariants of the item loop hipcc
        // computes dozens of them up front and spills them around the k-loop (the first build: 464 B of scratch per lane)
        int lane = lane_k;
        asm volatile("" : "+v"(lane));
        const int q = lane >> 4;
        const unsigned long long xb64 = reinterpret_cast<unsigned long long>(a.X + (size_t)f * L * DM);
        const unsigned long long wb64 = reinterpret_cast<unsigned long long>(a.W + (size_t)h * HD * DM);
        // fragment addresses: one opaque base register per (operand, stage, k-step) + an immediate per tile
        int fxa[2][2], fwa[2][2];
        {
            const int r7 = lane & 7, fbase = ((lane & 15) >> 3) * 1024 + r7 * 128;
#pragma unroll
            for (int st = 0; st < 2; ++st)
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    const int fkk = fbase + (((4 * kk + q) ^ r7) << 4);
                    fxa[st][kk] = st * STAGE_BYTES + wm * 5 * 2048 + fkk;
                    fwa[st][kk] = st * STAGE_BYTES + XP * 1024 + wn * 2 * 2048 + fkk;
                    asm volatile("" : "+v"(fxa[st][kk]), "+v"(fwa[st][kk]));
                }
        }
        f4 acc[6][5];
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j < 5; ++j) acc[i][j] = splat4(0.f);
        // this wave's feature tile i: kind i >> 1 (0 q, 1 k, 2 v), tile (i >> 1) 4 + wn 2 + (i & 1) of the head's 12
        constexpr int NK = DM / 64;
        static_assert(NK >= 2, "the prologue requests two k-tiles");      // an odd count (ViT-Tiny: 3) ends in stage 0, below
        const std::integral_constant<int, 0> S0{};
        const std::integral_constant<int, 1> S1{};
        auto SB = [&]() { __builtin_amdgcn_sched_barrier(0); };
        // ---- projection k-loop, software-pipelined; k-tile t lives in stage t & 1.  A k-tile is 12 GROUPS of 5 MFMAs: group g of half
        // H0 (k-step 0) / H1 (k-step 1) multiplies the wave's feature tile g with its five token tiles.  Registers: both k-steps' token
        // fragments (XA: k-step 0, XB: k-step 1) and a ROLLING window of three weight fragments (the stream (t, k0, 0..5), (t, k1, 0..5),
        // (t + 1, k0, 0..5) ...; element e + 2 is requested in group e) -- with all four fragment sets resident (88 registers) the loop
        // spilled its address registers and every reload drained the DMA queue (vmcnt).
        //     H0(t)   groups 0-5 on XA        | reads XB <- tile t k-step 1, weight stream          | DMA: W pieces of tile t + 1 (3 per wave, L2-resident:
        //                                                                                             they land within the half) -> other stage, groups 0-2
        //     Bm(t)   vmcnt(0) lgkmcnt(0), barrier: tile t + 1 has landed (its X pieces were issued a whole k-tile ago); this stage's X region is in registers
        //     H1(t)   groups 0-5 on XB        | reads XA <- tile t + 1 k-step 0, weight stream      | DMA: X pieces of tile t + 2 (5 per wave) -> this
        //                                                                                             stage's X region, groups 0-4
        //     Be(t)   lgkmcnt(0), barrier: this stage's W region is in registers (the next half's W DMA may overwrite it)
        // A region is written only behind the barrier that follows its last read; data is read only behind the barrier that follows the
        // wait that retires its DMA.
        auto dma = [&](int kt, int stg, int i) {                    // this wave's piece slot i (0-4: X, 5-7: W) of k-tile kt -> stage stg
            const int p = w + 8 * i;
            unsigned long long b64 = (i < 5 ? xb64 + (unsigned long long)i * (64ull * DM * 2) : wb64 + (unsigned long long)(i - 5) * ((unsigned long long)DM * DM * 2)) +
                                           (unsigned long long)kt * 128ull;
            if (VB_QA_DBG == 3 || VB_QA_DBG == 5) { if (i >= 5) b64 = reinterpret_cast<unsigned long long>(a.W) + (unsigned long long)(i - 5) * ((unsigned long long)DM * DM * 2); }
            if (VB_QA_DBG == 4 || VB_QA_DBG == 5) { if (i < 5) b64 = reinterpret_cast<unsigned long long>(a.X) + (unsigned long long)i * (64ull * DM * 2); }
            const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b64), hi = __builtin_amdgcn_readfirstlane((unsigned)(b64 >> 32));
            const char* base = reinterpret_cast<const char*>(((unsigned long long)hi << 32) | lo);
            unsigned off = soff;
            asm volatile("" : "+v"(off));
            if (VB_QA_DBG != 6) glds16(base + (size_t)off, smem + stg * STAGE_BYTES + p * 1024);
        };
        bf16x8 XA[5], XB[5], Wr[3];
        auto ldx = [&](auto stg, int kk, int j) { return *reinterpret_cast<const bf16x8*>(smem + fxa[decltype(stg)::value][kk] + j * 2048); };
        auto ldw = [&](auto stg, int kk, int i) { return *reinterpret_cast<const bf16x8*>(smem + fwa[decltype(stg)::value][kk] + ((i >> 1) * 4 + (i & 1)) * 2048); };
        auto mma5 = [&](int i, const bf16x8 (&fx)[5], const bf16x8 fw) {
            if (VB_QA_DBG == 7) return;
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                if (i >= 4) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fx[j], fw, acc[i][j], 0, 0, 0);     // v: tokens on rows
                else acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw, fx[j], acc[i][j], 0, 0, 0);
            }
        };
        auto ktile = [&](int kt, auto stg) {
            constexpr int ST = decltype(stg)::value;
            const std::integral_constant<int, ST ^ 1> nstg{};
#pragma unroll
            for (int g = 0; g < 6; ++g) {                 // H0: stream elements 0-5
                Wr[(g + 2) % 3] = g + 2 < 6 ? ldw(stg, 0, g + 2) : ldw(stg, 1, g + 2 - 6);
                if (g < 5) XB[g] = ldx(stg, 1, g);
                if (g < 3 && kt + 1 < NK) dma(kt + 1, ST ^ 1, 5 + g);
                SB();
                mma5(g, XA, Wr[g % 3]);
                SB();
            }
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            SB();
#pragma unroll
            for (int g = 0; g < 6; ++g) {                 // H1: stream elements 6-11
                if (g + 2 < 6) Wr[(6 + g + 2) % 3] = ldw(stg, 1, g + 2);
                else if (kt + 1 < NK) Wr[(6 + g + 2) % 3] = ldw(nstg, 0, g + 2 - 6);
                if (g < 5 && kt + 1 < NK) XA[g] = ldx(nstg, 0, g);
                if (g < 5 && kt + 2 < NK) dma(kt + 2, ST, g);
                SB();
                mma5(g, XB, Wr[(6 + g) % 3]);
                SB();
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            SB();
        };
        if (VB_QA_DBG != 2) {
#pragma unroll
            for (int i = 0; i < 8; ++i) dma(0, 0, i);
#pragma unroll
            for (int i = 0; i < 5; ++i) dma(1, 1, i);
            asm volatile("s_waitcnt vmcnt(5)" ::: "memory");         // tile 0 (8 pieces) has landed; tile 1's five X pieces stay in flight
            __builtin_amdgcn_s_barrier();
#pragma unroll
            for (int j = 0; j < 5; ++j) XA[j] = ldx(S0, 0, j);
            Wr[0] = ldw(S0, 0, 0);
            Wr[1] = ldw(S0, 0, 1);
            for (int kt = 0; kt + 1 < NK; kt += 2) {
                ktile(kt, S0);
                ktile(kt + 1, S1);
            }
            if constexpr (NK % 2 != 0) ktile(NK - 1, S0);      // (a k-tile asks for nothing beyond NK: its kt + 1 / kt + 2 tests)
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __syncthreads();
        // ---- epilogue: y = rstd * acc + bias, as bf16 into the attention's operand images (the stages are free: every wave has
        // passed the last k-tile's barrier)
        {
            int le = lane_k;
            asm volatile("" : "+v"(le));
            const int l15 = le & 15, q = le >> 4;
            float rs[5];            // q / k tiles: token tj 16 + l15
            f4 rs4[5];              // v tiles: tokens tj 16 + 4 q + {0..3}
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const int tj = wm * 5 + j;
                rs[j] = a.rstd ? a.rstd[(size_t)f * L + tj * 16 + l15] : 1.f;
                rs4[j] = a.rstd ? ld4(a.rstd + (size_t)f * L + tj * 16 + 4 * q) : splat4(1.f);
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const int ft = (i >> 1) * 4 + wn * 2 + (i & 1);      // 0-3 q, 4-7 k, 8-11 v
                if (ft < 8) {
                    const int nh = (ft & 3) * 16 + 4 * q;    // feature inside the head
                    const f4 bv = ld4(a.bias + (ft >> 2) * DM + h * HD + nh);
                    const int ks = nh >> 5, kb = (nh & 31) * 2;
#pragma unroll
                    for (int j = 0; j < 5; ++j) {
                        const int tj = wm * 5 + j, m = tj * 16 + l15;
                        const bf16x4 y = vbg::to_bf16x4(vbg::fma4(acc[i][j], splat4(rs[j]), bv));
                        if (ft < 4) {
                            *reinterpret_cast<bf16x4*>(Qimg + (tj * KS + ks) * 1024 + swz_byte(l15 * 64 + kb)) = y;
                        } else {           // K rows permuted: token m where the attention expects key m (the inverse of vba::perm_key)
                            const int t = vba::perm_tile(m), row = vba::perm_row(m);
                            *reinterpret_cast<bf16x4*>(Kimg + (t * KS + ks) * 1024 + swz_byte(row * 64 + kb)) = y;
                        }
                    }
                } else {
                    const int dt = ft - 8;                   // feature dt 16 + l15 of the head
                    const float bs = a.bias[2 * DM + h * HD + dt * 16 + l15];
#pragma unroll
                    for (int j = 0; j < 5; ++j) {
                        const int m = (wm * 5 + j) * 16 + 4 * q, c = m >> 5;
                        const bf16x4 y = vbg::to_bf16x4(vbg::fma4(acc[i][j], rs4[j], splat4(bs)));
                        *reinterpret_cast<bf16x4*>(Vimg + (dt * NC + c) * 1024 + swz_byte(l15 * 64 + (m & 31) * 2)) = y;
                    }
                }
            }
        }
        __syncthreads();
        // ---- attention of the frame's 20 query tiles: wave w takes tiles w, w + 8 (and w + 16 for w < 4); two tiles per pass
        auto pass = [&](auto nq_tag, int qt0, int qt1) {
            constexpr int NQ = decltype(nq_tag)::value;
            const int qts[2] = {qt0, qt1};
            int la = lane_k;
            asm volatile("" : "+v"(la));        // a fresh lane index per pass: keeps the K / V^T fragment reads (and the output addresses) inside it
            const int l15 = la & 15, q = la >> 4;
            const int frq = swz_byte(l15 * 64 + q * 16);          // fragment byte inside a 16 x 32 sub-tile of the images
            bf16x8 qf[NQ][KS];
#pragma unroll
            for (int u = 0; u < NQ; ++u)
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) qf[u][ks] = *reinterpret_cast<const bf16x8*>(Qimg + (qts[u] * KS + ks) * 1024 + frq);
            f4 S[NQ][NT];
            vba::qk_tiles(S, Kimg, frq, qf);
            float inv[NQ];
#pragma unroll
            for (int u = 0; u < NQ; ++u) {
                const float mx = quad_max(vba::lane_max(S[u]));
                inv[u] = 1.0f / quad_sum(vba::exp_rows(S[u], mx));
            }
            f4 O[NQ][DT];
#pragma unroll
            for (int u = 0; u < NQ; ++u)
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) O[u][dt] = splat4(0.f);
#pragma unroll
            for (int c = 0; c < NC; ++c) vba::pv_chunk(O, S, c, Vimg, NC, frq);
#pragma unroll
            for (int u = 0; u < NQ; ++u) vba::store_tile(a.out, (size_t)(f * L + qts[u] * 16 + l15), DM, h * HD + q * 4, O[u], inv[u]);
        };
        if (VB_QA_DBG != 1 && VB_QA_DBG < 3) {
            pass(std::integral_constant<int, 2>{}, w, w + 8);
            if (w < 4) pass(std::integral_constant<int, 1>{}, w + 16, 0);
        }
        __syncthreads();             // the images are dead: the next item's staging may overwrite them
    }
}

__global__ __launch_bounds__(512) void qkv_attn_kernel(const Args a) { qkv_attn_body<768>(a); }

// the same kernel at another width (ViT-Large: DM = 1024, 16 k-tiles, 16 heads; ViT-Small: 384, 6, 6; ViT-Tiny: 192, 3, 3)
template <int DM>
__global__ __launch_bounds__(512) void qkv_attn_wide_kernel(const Args a) { qkv_attn_body<DM>(a); }

}  // namespace vbq

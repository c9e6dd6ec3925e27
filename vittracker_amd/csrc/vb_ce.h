// vb_ce.h -- OSTrack candidate elimination (lib/models/layers/attn_blocks.py:20-85, lib/models/ostrack/vit_ce.py:151-186) by KEY MASKING
// and COMPACTED, gfx950.  The reference gathers the kept search tokens after the attention of blocks CE_LOC and runs the rest of the network on the
// shorter sequence.  A removed token can reach a later value of a kept one only as a key / value row of a later attention (LayerNorm, the
// MLP and every GEMM work per token), so here every matrix keeps its dense B x L rows, removed rows go on being computed and are never read
// by a kept row: later attentions take a per-frame key bitmap (vbs::attn_stream_masked_kernel) and the final norm's search rows of removed
// tokens are overwritten with zeros, as the reference's scatter into zeros does.  No token moves, no shape changes, nothing is faster.
// That is the MASKED form (VT_CE_MASKED, the default).  The COMPACT form (VT_CE_COMPACT, vt_set_ce_form) does what the reference does:
// behind a stage's selection the kept rows of every frame are gathered into a shorter dense frame -- template rows, kept search tokens in
// ascending global index, zero pad rows up to a multiple of 16 -- and every kernel behind it runs on B x Lp_k rows; the final norm scatters
// through the last index table to the tokens' global positions.  Same scores at the first removing stage (it runs before anything moves),
// same results, same tie rule.  Its kernels are at the end of this file; vbs::attn_stream_rt_kernel is its attention.
//
// The key bitmap of a frame: ceil(L / 32) uint32 words, bit (key & 31) of word (key >> 5) set = the key is present.  Template keys
// [0, Lz) are always present; bits at and past L are 0.  Stage k reads the bitmap stage k - 1 left (none: every key present) and writes its
// own, so a forward never has to reset anything; all buffers are indexed by absolute frame.
//
// Per stage, after the block's attention (the q | k rows the qk GEMM left in the workspace are still there):
//   ce_score_kernel    per (frame, head): sum over the selected template rows r of softmax_j(q_r . k_j) restricted to the present keys,
//                      for every search key -- attn[:, :, :lens_t, lens_t:] -> mask rows -> the sums of mean(2).mean(1).  bf16 q | k as
//                      the attention read them, logits / softmax / sums in f32, exp2 against the row maximum with the log2 e factor.
//                      PLAIN f32 loop for a selection of rows: the published configurations select ONE template row (CTR_POINT), 76 /
//                      188 us per launch at B = 256, a third / a quarter of the block's own attention.  CE_TEMPLATE_RANGE ALL (64 / 144
//                      rows) runs ce_score_all_kernel, the same sums on the bf16 MFMA (DESIGN.md 11.4 has both measured).
//   ce_select_kernel   per frame: the heads summed in head order and scaled to the mean, the rank of every present token among the
//                      present ones (ties: the lower index wins; the reference's torch.sort leaves them unspecified), the new bitmap,
//                      removed_stage and the stage's scores (NaN for tokens removed earlier).
// Every reduction has a fixed order (rows of a wave in row order, the four waves in wave order, heads in head order, wave reductions by
// butterfly): no float atomics, a score is a function of its frame's rows alone -- bit-identical run to run, eager and captured, in one
// chain or two.
#pragma once
#include "vb_attn.h"
#include "vb_misc.h"

namespace vbc {

using vbg::bf16;
using vbg::bf16x4;
using vbg::bf16x8;

constexpr int MAX_LX = 576;        // search tokens of the larger geometry (ce_select_kernel's LDS arrays)

__device__ __forceinline__ bool key_present(const uint32_t* fb, int key) { return !fb || ((fb[key >> 5] >> (key & 31)) & 1u); }

// The plain score of one (frame, head), under ce_score_kernel and ce_score_rt_kernel.  qf / kf: the head's q / k columns of the frame's first
// row, rows of 2 C; Lp: rows per frame; present(s): whether this lane's key lane + 64 s exists and is present (evaluated where it is used:
// the callers differ in what they precompute); red: [4][Lp] floats of LDS, the four waves' partial sums; out: [n], search keys Lz .. Lz + n.
// A wave takes rows w, w + 4, ...; a lane the keys lane, lane + 64, ... of every row.
template <int KPL, typename Present>
__device__ __forceinline__ void score_rows(const bf16* qf, const bf16* kf, int C, int Lp, const int32_t* __restrict__ rows, int nrows, Present present,
                                           float* red, int Lz, int n, float* __restrict__ out) {
    constexpr int HD = 64;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float acc[KPL];
#pragma unroll
    for (int s = 0; s < KPL; ++s) acc[s] = 0.f;
    for (int r = w; r < nrows; r += 4) {
        const bf16* qr = qf + (size_t)rows[r] * 2 * C;
        float qv[HD];
#pragma unroll
        for (int d = 0; d < HD; d += 8) {
            const bf16x8 t = *reinterpret_cast<const bf16x8*>(qr + d);
#pragma unroll
            for (int j = 0; j < 8; ++j) qv[d + j] = (float)t[j];
        }
        float sc[KPL], mx = -INFINITY;
#pragma unroll
        for (int s = 0; s < KPL; ++s) {
            sc[s] = -INFINITY;
            if (present(s)) {
                const bf16* kr = kf + (size_t)(lane + 64 * s) * 2 * C;
                float a = 0.f;
#pragma unroll
                for (int d = 0; d < HD; d += 8) {
                    const bf16x8 t = *reinterpret_cast<const bf16x8*>(kr + d);
#pragma unroll
                    for (int j = 0; j < 8; ++j) a = fmaf(qv[d + j], (float)t[j], a);
                }
                sc[s] = a;
            }
            mx = fmaxf(mx, sc[s]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));      // finite: the template keys are always present
        float sum = 0.f;
#pragma unroll
        for (int s = 0; s < KPL; ++s) {
            sc[s] = __builtin_amdgcn_exp2f((sc[s] - mx) * vba::LOG2E);           // an absent key: exp2(-inf) = 0
            sum += sc[s];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        const float inv = 1.0f / sum;
#pragma unroll
        for (int s = 0; s < KPL; ++s) acc[s] = fmaf(sc[s], inv, acc[s]);
    }
#pragma unroll
    for (int s = 0; s < KPL; ++s)
        if (lane + 64 * s < Lp) red[w * Lp + lane + 64 * s] = acc[s];
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += 256) out[j] = ((red[Lz + j] + red[Lp + Lz + j]) + red[2 * Lp + Lz + j]) + red[3 * Lp + Lz + j];
}

// grid = B * heads, 256 threads.  qk: [frame][L][2 C] bf16 (q pre-scaled | k); bits: [frame][ceil(L / 32)] or nullptr (every key present);
// rows: the nrows selected template rows; part: [frame][heads][L - Lz] f32, the sum over the rows of the softmax weights of the search keys.
template <int L>
__global__ __launch_bounds__(256) void ce_score_kernel(const bf16* __restrict__ qk, const uint32_t* __restrict__ bits,
                                                       const int32_t* __restrict__ rows, int nrows, float* __restrict__ part, int heads, int Lz) {
    constexpr int HD = 64, KPL = (L + 63) / 64, W = (L + 31) / 32;
    __shared__ float red[4][L];
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.x / heads, h = blockIdx.x - f * heads, C = heads * HD;
    const bf16* qf = qk + (size_t)f * L * 2 * C + h * HD;
    const uint32_t* fb = bits ? bits + (size_t)f * W : nullptr;
    bool ok[KPL];
#pragma unroll
    for (int s = 0; s < KPL; ++s) {
        const int key = lane + 64 * s;
        ok[s] = key < L && key_present(fb, key);
    }
    score_rows<KPL>(qf, qf + C, C, L, rows, nrows, [&](int s) { return ok[s]; }, &red[0][0], Lz, L - Lz, part + ((size_t)f * heads + h) * (L - Lz));
}

// ce_score_kernel's result for CE_TEMPLATE_RANGE ALL (every template row: Lz / 16 whole query tiles) on the 16x16x32 bf16 MFMA, of one
// (frame, head), under ce_score_all_kernel and ce_score_all_rt_kernel.  The plain loop above costs 3.3 x / 3.7 x the block's own attention
// there (64 / 144 rows: DESIGN.md 11.4); this form reads K once per query TILE.  qf, kf, Lp, Lz, n, out as score_rows, Lp / 16 whole key
// tiles; gone(t): 0 where this lane's key 16 t + (lane & 15) is present, else -inf; red: [16][Lp] floats of LDS; UNR: key
// tiles in flight per loop trip.  A wave takes query tiles w, w + 4, ..  S = Q K^T per 16-key tile: the q rows are the A operand and the k
// rows the B operand, both fetched from global memory with vba::load_q's addressing (row = lane & 15, k = 8 (lane >> 4) + {0..7}: the layout
// of either operand), so a lane holds S[query 16 qt + 4 (lane >> 4) + j][key 16 t + (lane & 15)], j = 0..3 -- a query's softmax runs along
// the lanes, the sum over queries along j and the four lane groups.  Two passes over the keys per query tile, nothing of size L in registers
// (the per-key accumulators live in LDS): pass 1 the online maximum and sum of each lane's column of keys, then combined over the 16 key
// lanes by butterfly; pass 2 the logits again, exp2 against the row maximum with the log2 e factor, times 1 / sum, added into the lane's
// accumulator of that key.  The 16 partial sums of a key (4 waves x 4 lane groups) meet in LDS in a fixed order.
template <int UNR, typename Gone>
__device__ __forceinline__ void score_all_tiles(const bf16* qf, const bf16* kf, int C, int Lp, Gone gone, float* red, int Lz, int n, float* __restrict__ out) {
    constexpr int HD = 64, KS = HD / 32;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, NT = Lp / 16;
    const int l15 = lane & 15, g = lane >> 4;
    // this lane's accumulator of key 16 t + l15 is red[4 w + g][16 t + l15]: its own slot, so the key loops need no unrolling (with the
    // accumulators in registers the compiler unrolls 45 tiles, hoists their loads and spills at L = 720)
    float* const acc = red + (size_t)(w * 4 + g) * Lp + l15;
    for (int t = 0; t < NT; ++t) acc[16 * t] = 0.f;
    // one key tile's logits of this lane's four queries; an absent key's column is -inf
    auto logits = [&](const bf16x8 (&qa)[KS], int t) {
        bf16x8 kb[KS];
        vba::load_q(kb, kf, t, l15, g, C);
        f4 S = splat4(0.f);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) S = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[ks], kb[ks], S, 0, 0, 0);
        // the MFMAs run for every lane, whatever gone() says, and -inf is ADDED: with `present ? S : -inf` the compiler put them inside the
        // branch on the lane's bit, and an MFMA under a partial EXEC mask returned wrong logits for every fifth tile
        return S + splat4(gone(t));
    };
    for (int qt = w; qt < Lz / 16; qt += 4) {
        bf16x8 qa[KS];
        vba::load_q(qa, qf, qt, l15, g, C);
        float m[4], l[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { m[j] = -1e30f; l[j] = 0.f; }      // finite: no inf - inf; the first present key sets it
#pragma unroll UNR
        for (int t = 0; t < NT; ++t) {
            const f4 S = logits(qa, t);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float mn = fmaxf(m[j], S[j]);
                l[j] = l[j] * __builtin_amdgcn_exp2f((m[j] - mn) * vba::LOG2E) + __builtin_amdgcn_exp2f((S[j] - mn) * vba::LOG2E);
                m[j] = mn;
            }
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1)      // over the 16 key lanes of a lane group
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float mo = __shfl_xor(m[j], o), lo = __shfl_xor(l[j], o), mn = fmaxf(m[j], mo);
                // two rounded products and a commutative add (no fma): both lanes of a pair get the same bits, so all 16 lanes end with
                // ONE normaliser and equal keys get equal scores bit for bit (the tie rule of ce_select_kernel is then what decides)
                {
#pragma clang fp contract(off)
                    const float mine = l[j] * __builtin_amdgcn_exp2f((m[j] - mn) * vba::LOG2E), theirs = lo * __builtin_amdgcn_exp2f((mo - mn) * vba::LOG2E);
                    l[j] = mine + theirs;
                }
                m[j] = mn;
            }
        float inv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) inv[j] = 1.0f / l[j];
#pragma unroll UNR
        for (int t = 0; t < NT; ++t) {
            const f4 S = logits(qa, t);
            float p[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) p[j] = __builtin_amdgcn_exp2f((S[j] - m[j]) * vba::LOG2E) * inv[j];
            acc[16 * t] += (p[0] + p[1]) + (p[2] + p[3]);
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += 256) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) s += red[(size_t)i * Lp + Lz + j];
        out[j] = s;
    }
}

// grid = B * heads, 256 threads; qk, bits, part as ce_score_kernel.
template <int L>
__global__ __launch_bounds__(256) void ce_score_all_kernel(const bf16* __restrict__ qk, const uint32_t* __restrict__ bits, float* __restrict__ part,
                                                           int heads, int Lz) {
    constexpr int HD = 64, NT = L / 16, W = (L + 31) / 32;
    static_assert(L % 16 == 0, "whole key tiles");
    constexpr int UNR = NT % 5 == 0 ? 5 : 1;      // key tiles in flight per loop trip (20 and 45 tiles: 5); more and L = 720 spills
    __shared__ float red[16][L];
    const int l15 = threadIdx.x & 15;
    const int f = blockIdx.x / heads, h = blockIdx.x - f * heads, C = heads * HD;
    const bf16* qf = qk + (size_t)f * L * 2 * C + h * HD;
    const uint32_t* fb = bits ? bits + (size_t)f * W : nullptr;
    auto gone = [&](int t) {      // a 16-key tile lies inside one word
        const uint32_t word = fb ? fb[t >> 1] : 0xffffffffu;
        return ((word >> ((16 * t + l15) & 31)) & 1u) ? 0.f : -INFINITY;
    };
    score_all_tiles<UNR>(qf, qf + C, C, L, gone, &red[0][0], Lz, L - Lz, part + ((size_t)f * heads + h) * (L - Lz));
}

// What the two select kernels share.  head_sum: candidate j's partial sums of frame f, [frame][heads][n], added in head order.  rank_of: how
// many of the n candidates that counts(i) admits stand before candidate j -- a higher score, or an equal one at a lower index.
__device__ __forceinline__ float head_sum(const float* __restrict__ part, int f, int heads, int n, int j) {
    float v = 0.f;
    for (int h = 0; h < heads; ++h) v += part[((size_t)f * heads + h) * n + j];
    return v;
}
template <typename Counts>
__device__ __forceinline__ int rank_of(const float* s, int n, int j, Counts counts) {
    const float sj = s[j];
    int rank = 0;
    for (int i = 0; i < n; ++i) {
        const float si = s[i];
        rank += (counts(i) && (si > sj || (si == sj && i < j))) ? 1 : 0;
    }
    return rank;
}

// grid = B, 256 threads.  part as ce_score_kernel left it; scale = 1 / (heads * nrows); prev: the bitmap this stage's attention ran under
// (nullptr: every key present -- then removed_stage is written for every token, else only for the tokens this stage removes); next: the
// bitmap after this stage; scores: [frame][Lx] of this stage.  keep: the stage's count of kept search tokens.
__global__ __launch_bounds__(256) void ce_select_kernel(const float* __restrict__ part, const uint32_t* __restrict__ prev, uint32_t* __restrict__ next,
                                                        uint8_t* __restrict__ removed, float* __restrict__ scores, int heads, float scale,
                                                        int stage, int keep, int L, int Lz) {
    __shared__ float s[MAX_LX];
    __shared__ uint8_t pres[MAX_LX], kept[MAX_LX];
    const int f = blockIdx.x, Lx = L - Lz, W = (L + 31) / 32;
    const uint32_t* fb = prev ? prev + (size_t)f * W : nullptr;
    for (int j = threadIdx.x; j < Lx; j += 256) {
        float v = head_sum(part, f, heads, Lx, j);
        const bool p = key_present(fb, Lz + j);
        v = p ? v * scale : __builtin_nanf("");
        s[j] = v;
        pres[j] = p;
        scores[(size_t)f * Lx + j] = v;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < Lx; j += 256) {
        bool k = false;
        if (pres[j]) {
            k = rank_of(s, Lx, j, [&](int i) { return pres[i] != 0; }) < keep;
            if (!k) removed[(size_t)f * Lx + j] = (uint8_t)stage;
            else if (!prev) removed[(size_t)f * Lx + j] = 0;
        }
        kept[j] = k;
    }
    __syncthreads();
    for (int w = threadIdx.x; w < W; w += 256) {
        uint32_t word = 0;
        for (int b = 0; b < 32; ++b) {
            const int key = 32 * w + b;
            if (key < Lz || (key < L && kept[key - Lz])) word |= 1u << b;
        }
        next[(size_t)f * W + w] = word;
    }
}

// The reference returns zeros for the removed tokens (vit_ce.py:170-181 scatters the kept rows into zeros after the final norm): the
// search rows of absent keys in the head's padded input map [frame][F + 2][F + 2][C] and in feat [frame][Lx][C] (optional) become exact
// zeros.  Grid-stride over (frame, search token, 4 channels).
__global__ __launch_bounds__(256) void ce_zero_rows_kernel(const uint32_t* __restrict__ bits, bf16* __restrict__ map, float* __restrict__ feat, int B, int L,
                                                           int Lz, int F, int C) {
    const int Lx = L - Lz, W = (L + 31) / 32, C4 = C / 4;
    const size_t total = (size_t)B * Lx * C4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % C4) * 4;
        const size_t row = i / C4;
        const int t = (int)(row % Lx), f = (int)(row / Lx);
        if (key_present(bits + (size_t)f * W, Lz + t)) continue;
        const int y = t / F, x = t - y * F;
        *reinterpret_cast<bf16x4*>(map + vbm::map_px(f, y, x, F, C) + c) = bf16x4{(bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f};
        if (feat) st4(feat + row * C + c, splat4(0.f));
    }
}

// ------------------------------------------------------------------------------------------------ the COMPACT form
// Behind a stage's selection the kept tokens of every frame are gathered into a shorter dense sequence and everything behind it runs on
// B x Lp rows (header comment).  A compacted frame: Lz template rows, the kept search tokens in ascending GLOBAL index, then pad rows up
// to Lp = round_up(Lz + kept, 16).  Pad rows are zero-filled by the gather, never present as keys (nkeys = Lz + kept is a plain count) and
// never read.  index [frame][kept]: the global search index of compacted search row i; inv [frame][Lx]: the compacted search row of a
// global token, -1 = removed.  The kernels below take the frame length at run time.

// ce_score_kernel at a run-time frame length: Lp rows per frame, keys [0, nkeys) present.  KPL: keys per lane, 64 KPL >= Lp.  grid = B * heads,
// 256 threads, 4 * Lp floats of dynamic LDS; part: [frame][heads][nkeys - Lz].
template <int KPL>
__global__ __launch_bounds__(256) void ce_score_rt_kernel(const bf16* __restrict__ qk, int Lp, int nkeys, const int32_t* __restrict__ rows, int nrows,
                                                          float* __restrict__ part, int heads, int Lz) {
    constexpr int HD = 64;
    extern __shared__ float red_rt[];      // [4][Lp]
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.x / heads, h = blockIdx.x - f * heads, C = heads * HD;
    const bf16* qf = qk + (size_t)f * Lp * 2 * C + h * HD;
    const int n = nkeys - Lz;
    score_rows<KPL>(qf, qf + C, C, Lp, rows, nrows, [&](int s) { return lane + 64 * s < nkeys; }, red_rt, Lz, n, part + ((size_t)f * heads + h) * n);
}

// ce_score_all_kernel at a run-time frame length (every template row, on the MFMA).  grid = B * heads, 256 threads, 16 * Lp floats of dynamic
// LDS.  The pad keys lie in the last key tile.
__global__ __launch_bounds__(256) void ce_score_all_rt_kernel(const bf16* __restrict__ qk, int Lp, int nkeys, float* __restrict__ part, int heads, int Lz) {
    constexpr int HD = 64;
    extern __shared__ float red_rt[];      // [16][Lp]
    const int l15 = threadIdx.x & 15;
    const int f = blockIdx.x / heads, h = blockIdx.x - f * heads, C = heads * HD;
    const bf16* qf = qk + (size_t)f * Lp * 2 * C + h * HD;
    const int n = nkeys - Lz;
    score_all_tiles<1>(qf, qf + C, C, Lp, [&](int t) { return 16 * t + l15 < nkeys ? 0.f : -INFINITY; }, red_rt, Lz, n,
                       part + ((size_t)f * heads + h) * n);
}

// Select on the current candidates.  grid = B, 256 threads.  part: [frame][heads][ncand], candidate i of a frame being global search token
// prev[frame][i] (prev == nullptr: the uncompacted frame, candidate i = token i).  Ranks the ncand candidates (ties: the lower GLOBAL index wins
// -- candidates stand in ascending global index, so the lower candidate does) and writes, all at GLOBAL positions: the stage's scores (NaN for
// tokens removed before), removed_stage, inv; and per kept token, in ascending order: next[frame][j] its global index, src[frame][j] its
// candidate number (what the gather reads).
__global__ __launch_bounds__(256) void ce_select_compact_kernel(const float* __restrict__ part, const int32_t* __restrict__ prev, int32_t* __restrict__ next,
                                                                int32_t* __restrict__ src, int32_t* __restrict__ inv, uint8_t* __restrict__ removed,
                                                                float* __restrict__ scores, int heads, float scale, int stage, int ncand, int keep, int Lx) {
    __shared__ float s[MAX_LX];
    __shared__ uint8_t kept[MAX_LX];
    __shared__ int wsum[4];
    const int f = blockIdx.x;
    const int32_t* pf = prev ? prev + (size_t)f * ncand : nullptr;
    for (int j = threadIdx.x; j < Lx; j += 256) {
        if (pf) scores[(size_t)f * Lx + j] = __builtin_nanf("");
        inv[(size_t)f * Lx + j] = -1;
    }
    for (int j = threadIdx.x; j < ncand; j += 256) {
        s[j] = head_sum(part, f, heads, ncand, j) * scale;
    }
    __syncthreads();      // also orders the NaN / -1 fill before the writes below (the same block, global memory)
    for (int j = threadIdx.x; j < ncand; j += 256) {
        const float sj = s[j];
        const bool k = rank_of(s, ncand, j, [](int) { return true; }) < keep;
        const int gidx = pf ? pf[j] : j;
        scores[(size_t)f * Lx + gidx] = sj;
        if (!k) removed[(size_t)f * Lx + gidx] = (uint8_t)stage;
        else if (!pf) removed[(size_t)f * Lx + gidx] = 0;
        kept[j] = k;
    }
    __syncthreads();
    // stable compaction: thread t owns candidates [t * per, (t + 1) * per); exclusive prefix of the kept counts over the threads
    const int per = (ncand + 255) / 256, j0 = threadIdx.x * per, j1 = min(ncand, j0 + per);
    int cnt = 0;
    for (int j = j0; j < j1; ++j) cnt += kept[j];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    int pos = incl - cnt;
    for (int i = 0; i < w; ++i) pos += wsum[i];
    for (int j = j0; j < j1; ++j)
        if (kept[j] && pos < keep) {      // pos < keep always, but for NaN scores (every rank 0): the tables' bounds hold whatever the input
            const int gidx = pf ? pf[j] : j;
            next[(size_t)f * keep + pos] = gidx;
            src[(size_t)f * Lx + pos] = j;
            inv[(size_t)f * Lx + gidx] = pos;
            ++pos;
        }
}

// The gather behind select: frame f's new row i is template row i (i < Lz), candidate src[f][i - Lz] (i < Lz + keep) or a zero pad row.
// Source rows at stride Lsrc, destination rows at stride Ldst, in OTHER buffers (frames run in parallel and frame f's destination would
// overlap earlier frames' sources in place).  Moves the attention output (bf16), the residual stream (f32) and the rows' centring mean.
// One wave per row, 4 rows per block; C a multiple of 256.
__global__ __launch_bounds__(256) void ce_gather_kernel(const bf16* __restrict__ ao, const float* __restrict__ resid, const float* __restrict__ rmean,
                                                        const int32_t* __restrict__ src, bf16* __restrict__ ao_out, float* __restrict__ resid_out,
                                                        float* __restrict__ rmean_out, int B, int Lsrc, int Ldst, int Lz, int keep, int Lx, int C) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long long)B * Ldst) return;
    const int f = (int)(row / Ldst), i = (int)(row - (long long)f * Ldst);
    const bool live = i < Lz + keep;
    const size_t from = (size_t)f * Lsrc + (i < Lz ? i : (live ? Lz + src[(size_t)f * Lx + i - Lz] : 0));
    for (int c = lane * 4; c < C; c += 256) {
        const bf16x4 z4 = {(bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f};
        *reinterpret_cast<bf16x4*>(ao_out + (size_t)row * C + c) = live ? *reinterpret_cast<const bf16x4*>(ao + from * C + c) : z4;
        st4(resid_out + (size_t)row * C + c, live ? ld4(resid + from * C + c) : splat4(0.f));
    }
    if (lane == 0) rmean_out[row] = live ? rmean[from] : 0.f;
}

// The final LayerNorm on compacted rows, scattered to the tokens' global positions: one wave per (frame, global search token).  A kept token
// (inv >= 0) is row f * Lp + Lz + inv of resid: its norm goes to the head's padded map and to feat (optional), as vbm::layernorm_kernel
// writes them; a removed token's row of both is exactly zero (vit_ce.py:170-181).  Every interior row is written once; the border is not touched.
template <int C>
__global__ __launch_bounds__(256) void ce_final_norm_kernel(const float* __restrict__ resid, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            float eps, const int32_t* __restrict__ inv, int B, int Lp, int Lz, int Lx, int F,
                                                            bf16* __restrict__ map, float* __restrict__ feat) {
    constexpr int NV = vbm::ln_slots<C, 4>();
    const int lane = threadIdx.x & 63;
    const long long o = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= (long long)B * Lx) return;
    const int f = (int)(o / Lx), tt = (int)(o - (long long)f * Lx);
    const int p = inv[o];
    f4 y[NV];
    if (p >= 0) {
        const vbm::LnStats st = vbm::ln_row<C, 4, false>(resid + ((size_t)f * Lp + Lz + p) * C, lane, eps, y, [](int, int, f4) {});
#pragma unroll
        for (int i = 0; i < NV; ++i) y[i] = vbm::ln_affine<4>(y[i], st.rstd, gamma, beta, vbm::ln_col<4>(i, lane));
    } else {
#pragma unroll
        for (int i = 0; i < NV; ++i) y[i] = splat4(0.f);
    }
    const int yy = tt / F, xx = tt - yy * F;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = vbm::ln_col<4>(i, lane);
        *reinterpret_cast<bf16x4*>(map + vbm::map_px(f, yy, xx, F, C) + c) = vbg::to_bf16x4(y[i]);
        if (feat) st4(feat + (size_t)o * C + c, y[i]);
    }
}

// Compacted f32 rows back to the dense (B, L, C) layout (vb::blocks' resid_out): template rows as they are, kept search rows at their
// global positions, removed rows zero.  One wave per destination row.
__global__ __launch_bounds__(256) void ce_scatter_rows_kernel(const float* __restrict__ resid, const int32_t* __restrict__ inv, float* __restrict__ out, int B,
                                                              int Lp, int L, int Lz, int C) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long long)B * L) return;
    const int f = (int)(row / L), t = (int)(row - (long long)f * L);
    const int p = t < Lz ? t : inv[(size_t)f * (L - Lz) + t - Lz];
    const float* r = resid + ((size_t)f * Lp + (t < Lz ? t : Lz + p)) * C;
    for (int c = lane * 4; c < C; c += 256) st4(out + (size_t)row * C + c, p >= 0 ? ld4(r + c) : splat4(0.f));
}

}  // namespace vbc

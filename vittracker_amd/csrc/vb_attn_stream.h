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

}  // namespace vbs

// vb_misc.h -- the HBM-bound kernels around the GEMMs of the ViT-Base path: patch gathering, LayerNorm, head tail.
#pragma once
#include "vb_gemm.h"
#include "vt_bf3.h"

namespace vbm {

using vbg::bf16;
using vbg::bf16x4;
using vbg::bf16x8;

// Element offset of pixel (y, x) of frame b in a zero-bordered NHWC map [B][F + 2][F + 2][C]: the head's implicit-GEMM inputs (C: the
// channels of a pixel as the map stores them -- 6 C for a map of expanded pixels, vb_f32.h)
__device__ __forceinline__ size_t map_px(int b, int y, int x, int F, int C) {
    const int P = F + 2;
    return ((size_t)(b * P + y + 1) * P + x + 1) * C;
}

// ---------------------------------------------------------------------------------------------- patches
// PatchEmbed's Conv2d(3, C, 16, stride 16) (lib/models/layers/patch_embed.py:20-32) as a GEMM whose left operand is the crops' patches,
// P[m = frame * tokens + token][k = c * 256 + r * 16 + s] (k order = the conv weight's own [3][16][16] order).  A row is walked as 96
// chunks of 8 consecutive s: chunk ch = c * 32 + r * 2 + (s >> 3).  crop_patch_src: where chunk ch of token t of frame f starts in an fp32
// crop batch (B, 3, T, T) of g = T / 16 tokens a side.
__device__ __forceinline__ const float* crop_patch_src(const float* img, int T, int g, int f, int t, size_t ch) {
    const int c = ch >> 5, r = (ch >> 1) & 15, s0 = (ch & 1) * 8, py = t / g, px = t - py * g;
    return img + (((size_t)f * 3 + c) * T + py * 16 + r) * T + px * 16 + s0;
}

// The combined operand in bf16, template tokens first (combine_tokens 'direct', lib/models/ostrack/utils.py:13-14).
// One thread = 8 consecutive s of one (m, c, r): 32 B in, 16 B out, writes fully coalesced.
__global__ __launch_bounds__(256) void patchify_kernel(const float* __restrict__ z, const float* __restrict__ x,
                                                       bf16* __restrict__ P, int B, int Tz, int Tx) {
    const int gz = Tz / 16, gx = Tx / 16, Lz = gz * gz, L = Lz + gx * gx;
    const size_t total = (size_t)B * L * 96;                    // 96 = 3 * 16 * 2 chunks of 8 per patch
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int ch = (int)(i % 96);
        const size_t m = i / 96;
        const int t = (int)(m % L), f = (int)(m / L);
        const float* src;
        if (t < Lz) src = crop_patch_src(z, Tz, gz, f, t, ch);
        else src = crop_patch_src(x, Tx, gx, f, t - Lz, ch);
        const bf16x4 lo = vbg::to_bf16x4(ld4(src)), hi = vbg::to_bf16x4(ld4(src + 4));
        *reinterpret_cast<bf16x8*>(P + m * 768 + ch * 8) = bf16x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    }
}

// One pixel row of one token of the uint8 HWC patch (B, T, T, 3) that vt_crop_u8* writes (sample_target's output): row r of operand row
// m = frame * Lx + token (g = T / 16 tokens a side, Lx = g * g).  48 contiguous bytes in (offset a multiple of 48: three aligned 16-byte
// nontemporal loads); per channel c, the row's 16 values bf16(byte - centre) as eight packed pairs go to store(c, first four, last four).
// |byte - centre| has at most 8 significant bits: its bf16 is exact, the conversion is the float's upper half.
template <typename Store>
__device__ __forceinline__ void u8_row_unpack(const unsigned char* __restrict__ xp, int T, int g, int Lx, size_t m, int r, float centre, Store&& store) {
    using vbg::u32x4;
    const int t = (int)(m % Lx), py = t / g, px = t - py * g;
    const size_t f = m / Lx;
    const u32x4* src = reinterpret_cast<const u32x4*>(xp + ((f * T + py * 16 + r) * T + px * 16) * 3);
    unsigned w[12];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const u32x4 v = __builtin_nontemporal_load(src + j);
        w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        unsigned o[8];
#pragma unroll
        for (int s = 0; s < 16; s += 2) {      // byte 3 s + c of the row: channel c of pixel s (v_cvt_f32_ubyteN picks it out of its dword)
            const int k0 = 3 * s + c, k1 = k0 + 3;
            const float v0 = (float)((w[k0 >> 2] >> (8 * (k0 & 3))) & 255u) - centre;
            const float v1 = (float)((w[k1 >> 2] >> (8 * (k1 & 3))) & 255u) - centre;
            o[s >> 1] = __builtin_amdgcn_perm(__float_as_uint(v1), __float_as_uint(v0), 0x07060302u);      // v_perm: the two upper halves
        }
        store(c, u32x4{o[0], o[1], o[2], o[3]}, u32x4{o[4], o[5], o[6], o[7]});
    }
}

// The search rows of the operand from the uint8 patch, DENSE: P[m][k = c * 256 + r * 16 + s] = bf16(byte - centre).  Preprocessor.process's
// / 255, - mean, / std live in the weights this operand meets (vitb.hip fold_preprocessor); centre = 128 takes the bytes' common mode out of
// what those rounded weights multiply.  One thread = pixel row r of one token, one 32-byte run out per channel.  r is the fastest lane
// index, so the 16 lanes of a token write each channel's 16 runs as ONE contiguous 512 bytes.
__global__ __launch_bounds__(256) void patchify_u8_kernel(const unsigned char* __restrict__ xp, bf16* __restrict__ P, int B, int T, float centre) {
    const int g = T / 16, Lx = g * g;
    const size_t total = (size_t)B * Lx * 16;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int r = (int)(i & 15);
        const size_t m = i >> 4;
        u8_row_unpack(xp, T, g, Lx, m, r, centre, [&](int c, vbg::u32x4 lo, vbg::u32x4 hi) {
            vbg::u32x4* dst = reinterpret_cast<vbg::u32x4*>(P + m * 768 + c * 256 + r * 16);
            dst[0] = lo;
            dst[1] = hi;
        });
    }
}

// -------------------------------------------------------------------------------------------- LayerNorm
// nn.LayerNorm(C, eps) of one row of the f32 residual stream (lib/models/ostrack/vit.py:78,82,130; eps 1e-6) by one wave: biased variance,
// two passes over registers.  The 64 lanes hold the row as slots of VW floats: slot i of a lane is columns (i * 64 + lane) * VW ..., so a wave
// reads and writes whole contiguous runs of 64 VW floats.  VW = 4 (float4) at C a multiple of 256, or at any C a multiple of 4 with MASK:
// the last slot's upper lanes then hold nothing and add zeros to the sums; VW = 2 / 1 at a multiple of 128 / 64, every lane active.
template <int VW> struct LnVec;
template <> struct LnVec<1> { typedef float f; typedef bf16 b; };
template <> struct LnVec<2> { typedef vbg::f2 f; typedef vbg::bf16x2 b; };
template <> struct LnVec<4> { typedef f4 f; typedef bf16x4 b; };
template <int VW>
__device__ __forceinline__ float ln_hsum(typename LnVec<VW>::f v) {
    if constexpr (VW == 4) return hsum4(v);
    else if constexpr (VW == 2) return v.x + v.y;
    else return v;
}
template <int VW>
__device__ __forceinline__ typename LnVec<VW>::b ln_to_bf16(typename LnVec<VW>::f v) {
    if constexpr (VW == 4) return vbg::to_bf16x4(v);
    else if constexpr (VW == 2) return __builtin_convertvector(v, vbg::bf16x2);
    else return (bf16)v;
}
template <int VW>
__device__ __forceinline__ typename LnVec<VW>::f ln_load(const float* p) { return *reinterpret_cast<const typename LnVec<VW>::f*>(p); }
template <int C, int VW>
constexpr int ln_slots() { return (C + 64 * VW - 1) / (64 * VW); }
template <int VW>
__device__ __forceinline__ int ln_col(int i, int lane) { return (i * 64 + lane) * VW; }

// The row body: loads row p into v, leaves v CENTRED (x - mean; a masked-off slot stays zero) and returns mean and 1 / sqrt(var + eps).
// centred(i, c, v[i]) is called on every live slot as it is centred (column c).
struct LnStats { float mean, rstd; };
template <int C, int VW, bool MASK, typename Slot>
__device__ __forceinline__ LnStats ln_row(const float* __restrict__ p, int lane, float eps, typename LnVec<VW>::f (&v)[ln_slots<C, VW>()], Slot&& centred) {
    static_assert(MASK ? C % VW == 0 : C % (64 * VW) == 0, "C = 64 lanes x VW floats x n, or a masked last slot");
    constexpr int NV = ln_slots<C, VW>();
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = ln_col<VW>(i, lane);
        v[i] = (!MASK || c < C) ? ln_load<VW>(p + c) : typename LnVec<VW>::f{};
        s += ln_hsum<VW>(v[i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s * (1.0f / C);
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = ln_col<VW>(i, lane);
        if (!MASK || c < C) {
            v[i] = v[i] - mean;
            ss += ln_hsum<VW>(v[i] * v[i]);
            centred(i, c, v[i]);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    return {mean, 1.0f / sqrtf(ss * (1.0f / C) + eps)};
}
// a centred slot at column c -> its normalised value
template <int VW>
__device__ __forceinline__ typename LnVec<VW>::f ln_affine(typename LnVec<VW>::f v, float rstd, const float* __restrict__ gamma, const float* __restrict__ beta, int c) {
    return v * rstd * ln_load<VW>(gamma + c) + ln_load<VW>(beta + c);
}

// LayerNorm over the residual stream, one wave per token row, 4 rows per block:
//   xn   (optional)  bf16 [M][C]                                   -> the next GEMM's left operand
//   map  (optional)  bf16 zero-bordered NHWC [B][F+2][F+2][C]: search rows only (forward_head's (B,C,F,F) view,
//                    lib/models/ostrack/ostrack.py:126-129)         -> the head's implicit-GEMM input
//   feat (optional)  f32 [B][Lx][C]: search rows only               -> stage API / tests
//   xb + rstd (optional, together)  the LayerNorm folded into the next GEMM (vb_gemm.h): bf16 copy of the RAW row and its
//                    1 / sqrt(var + eps) -- what the residual-writing GEMM epilogues + ln_finalize_kernel produce, for a
//                    residual stream that arrived from outside (vt_blocks on caller-supplied tokens)
template <int C, int VW>
__device__ __forceinline__ void layernorm_rows(const float* __restrict__ resid, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                               int M, int L, int Lz, int F, bf16* __restrict__ xn, bf16* __restrict__ map, float* __restrict__ feat,
                                               bf16* __restrict__ xb, float* __restrict__ rstd_out, float* __restrict__ mean_out) {
    typedef typename LnVec<VW>::f fv;
    typedef typename LnVec<VW>::b bv;
    constexpr int NV = ln_slots<C, VW>();
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    fv v[NV];
    // the raw rows' bf16 copy for the LayerNorm-folded GEMMs, CENTRED (vb_gemm.h Args::cm): the folded weights ignore a per-row constant
    const LnStats st = ln_row<C, VW, false>(resid + (size_t)row * C, lane, eps, v, [&](int, int c, fv x) {
        if (xb) *reinterpret_cast<bv*>(xb + (size_t)row * C + c) = ln_to_bf16<VW>(x);
    });
    if (rstd_out) {
        if (lane == 0) { rstd_out[row] = st.rstd; if (mean_out) mean_out[row] = st.mean; }
        if (!xn && !map && !feat) return;
    }
    const int f = row / L, t = row - f * L;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = ln_col<VW>(i, lane);
        const fv y = ln_affine<VW>(v[i], st.rstd, gamma, beta, c);
        if (xn) *reinterpret_cast<bv*>(xn + (size_t)row * C + c) = ln_to_bf16<VW>(y);
        if (t >= Lz) {
            const int tt = t - Lz;
            if (map) {
                const int yy = tt / F, xx = tt - yy * F;
                *reinterpret_cast<bv*>(map + map_px(f, yy, xx, F, C) + c) = ln_to_bf16<VW>(y);
            }
            if (feat) *reinterpret_cast<fv*>(feat + ((size_t)f * (L - Lz) + tt) * C + c) = y;
        }
    }
}

// C = 768 = 64 lanes x 3 float4 (and 1024)
template <int C>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ resid, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float eps, int M, int L, int Lz, int F,
                                                        bf16* __restrict__ xn, bf16* __restrict__ map, float* __restrict__ feat,
                                                        bf16* __restrict__ xb, float* __restrict__ rstd_out, float* __restrict__ mean_out) {
    static_assert(C % 256 == 0, "C = 64 lanes x float4 x n");
    layernorm_rows<C, 4>(resid, gamma, beta, eps, M, L, Lz, F, xn, map, feat, xb, rstd_out, mean_out);
}

// The same LayerNorm at a width that is no multiple of 256 (ViT-Small 384, ViT-Tiny 192): float2 lanes at a multiple of 128, else float (C a
// multiple of 64).  All 64 lanes are active, so the butterfly sums no padding.  Its own kernel: layernorm_kernel<768 / 1024> keep their code.
template <int C>
__global__ __launch_bounds__(256) void layernorm_small_kernel(const float* __restrict__ resid, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps, int M, int L, int Lz, int F,
                                                              bf16* __restrict__ xn, bf16* __restrict__ map, float* __restrict__ feat,
                                                              bf16* __restrict__ xb, float* __restrict__ rstd_out, float* __restrict__ mean_out) {
    static_assert(C % 64 == 0 && C % 256 != 0, "C = 64 lanes x (float2 | float) x n; multiples of 256 take layernorm_kernel");
    layernorm_rows<C, C % 128 == 0 ? 2 : 1>(resid, gamma, beta, eps, M, L, Lz, F, xn, map, feat, xb, rstd_out, mean_out);
}

// ------------------------------------------------------------------------- the fp32-equivalent mode
// An fp32 operand of a GEMM is stored as its three exact bf16 pieces x = h + m + l (split3_rne below), laid out along k as the six k-ranges
// [xm | xh | xl | xh | xm | xh] of an expanded row of 6 K; the weight row is [wm | wl | wh | wm | wh | wh] (vb_f32.h expand_weight_kernel).
// vbg::gemm_kernel at depth 6 K then sums mm, hl, lh, hm, mh, hh in that order: the small terms meet the accumulator first.
// split3_rne: h = bf16(x), m = bf16(x - h), l = bf16(x - h - m), each rounded to nearest even (v_cvt_pk_bf16_f32); both subtractions are
// exact and the last residual has at most 8 significant bits, so x = h + m + l exactly, as with vt3::split3's truncation.  Rounded pieces
// are half the size of truncated ones and of either sign: the three dropped cross terms (ml, lm, ll) are below 2^-26 of a product and
// unbiased, where truncation's are up to 2^-24 and all of the product's sign -- measured on three fixtures, the worst ratio of the device's
// error to the reference's own fp32 error fell from 8.5 to 5.0.  Same pair packing as vt3::split3: element r in the low half first.
__device__ __forceinline__ void split3_rne(f4 x, vt3::u32x2& h, vt3::u32x2& m, vt3::u32x2& l) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const vbg::f2 v = {x[2 * p], x[2 * p + 1]};
        const unsigned hu = __builtin_bit_cast(unsigned, __builtin_convertvector(v, vbg::bf16x2));
        const vbg::f2 r1 = v - vbg::f2{__uint_as_float(hu << 16), __uint_as_float(hu & 0xffff0000u)};
        const unsigned mu = __builtin_bit_cast(unsigned, __builtin_convertvector(r1, vbg::bf16x2));
        const vbg::f2 r2 = r1 - vbg::f2{__uint_as_float(mu << 16), __uint_as_float(mu & 0xffff0000u)};
        h[p] = hu; m[p] = mu; l[p] = __builtin_bit_cast(unsigned, __builtin_convertvector(r2, vbg::bf16x2));
    }
}
// store_split8: eight values at column c (a multiple of 8) of a K-wide row, as six 16-byte stores into the expanded row `row`.
__device__ __forceinline__ void store_split8(bf16* row, int K, int c, f4 a, f4 b) {
    vt3::u32x2 ha, ma, la, hb, mb, lb;
    split3_rne(a, ha, ma, la);
    split3_rne(b, hb, mb, lb);
    const vt3::u32x4 h = vt3::cat2(ha, hb), m = vt3::cat2(ma, mb), l = vt3::cat2(la, lb);
    vt3::u32x4* p = reinterpret_cast<vt3::u32x4*>(row + c);
    const int s = K / 8;      // a k-range in 16-byte units
    p[0] = m; p[s] = h; p[2 * s] = l; p[3 * s] = h; p[4 * s] = m; p[5 * s] = h;
}
__device__ __forceinline__ void store_split4(bf16* row, int K, int c, f4 a) {      // four values, 8-byte stores
    vt3::u32x2 h, m, l;
    split3_rne(a, h, m, l);
    vt3::u32x2* p = reinterpret_cast<vt3::u32x2*>(row + c);
    const int s = K / 4;
    p[0] = m; p[s] = h; p[2 * s] = l; p[3 * s] = h; p[4 * s] = m; p[5 * s] = h;
}

// LayerNorm over the f32 residual stream with f32 statistics, one wave per row, writing the next GEMM's expanded operand xs [M][6 C]
// and / or the search rows as f32 feat [B][Lx][C] (the final norm).  Lanes hold float4 slots of 256 columns; at widths that are no multiple
// of 256 (384, 192) the last slot's upper lanes hold nothing and add zeros to the sums.
template <int C>
__global__ __launch_bounds__(256) void layernorm_split_kernel(const float* __restrict__ resid, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps, int M, int L, int Lz,
                                                              bf16* __restrict__ xs, float* __restrict__ feat) {
    constexpr int NV = ln_slots<C, 4>();
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    f4 v[NV];
    const LnStats st = ln_row<C, 4, C % 256 != 0>(resid + (size_t)row * C, lane, eps, v, [](int, int, f4) {});
    const int f = row / L, t = row - f * L;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = ln_col<4>(i, lane);
        if (c >= C) continue;
        const f4 y = ln_affine<4>(v[i], st.rstd, gamma, beta, c);
        if (xs) store_split4(xs + (size_t)row * 6 * C, C, c, y);
        if (feat && t >= Lz) st4(feat + ((size_t)f * (L - Lz) + (t - Lz)) * C + c, y);
    }
}

// nn.GELU() in its exact erf form on the f32 pre-activation [rows][N], written as fc2's expanded operand [rows][6 N].  One thread = 8 columns
__device__ __forceinline__ float gelu_erf(float u) { return 0.5f * u * (1.0f + erff(u * 0.70710678118654752440f)); }
__global__ __launch_bounds__(256) void gelu_split_kernel(const float* __restrict__ pre, bf16* __restrict__ xs, size_t rows, int N) {
    const size_t per = (size_t)N / 8, total = rows * per;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t r = i / per;
        const int c = (int)(i - r * per) * 8;
        const f4 a = ld4(pre + r * N + c), b = ld4(pre + r * N + c + 4);
        store_split8(xs + r * 6 * N, N, c, f4{gelu_erf(a.x), gelu_erf(a.y), gelu_erf(a.z), gelu_erf(a.w)},
                     f4{gelu_erf(b.x), gelu_erf(b.y), gelu_erf(b.z), gelu_erf(b.w)});
    }
}

// Per-row rstd from the (sum, centred sum of squares) pairs the residual-writing GEMM epilogues leave per 64-column wave slice
// (vb_gemm.h): Chan's pairwise update, exact mean first.  stats: [P][ld] float2, P = C / 64.  One thread per row.
template <int P>
__global__ __launch_bounds__(256) void ln_finalize_kernel(const vbg::f2* __restrict__ stats, int ld, int M, float eps, float* __restrict__ rstd,
                                                          float* __restrict__ mean_out) {      // mean_out: the next residual-writing GEMM centres its bf16 copy on it
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    vbg::f2 v[P];           // all P pairs requested at once: one memory round trip per row
#pragma unroll
    for (int p = 0; p < P; ++p) v[p] = stats[(size_t)p * ld + m];
    float s = 0.f;
#pragma unroll
    for (int p = 0; p < P; ++p) s += v[p].x;
    const float inv_c = 1.0f / (64.0f * P), mean = s * inv_c;
    float m2 = 0.f;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const float d = v[p].x * (1.0f / 64.0f) - mean;
        m2 += v[p].y + 64.0f * d * d;
    }
    rstd[m] = 1.0f / sqrtf(m2 * inv_c + eps);
    if (mean_out) mean_out[m] = mean;
}

// f32 (B, Lx, C) tokens -> the zero-bordered bf16 map (stage API: vt_head on caller-supplied features)
__global__ __launch_bounds__(256) void feat_to_map_kernel(const float* __restrict__ feat, bf16* __restrict__ map, int B, int F, int C) {
    const size_t total = (size_t)B * F * F * (C / 4);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % (C / 4)) * 4;
        const size_t px = i / (C / 4);
        const int x = (int)(px % F), y = (int)((px / F) % F), b = (int)(px / ((size_t)F * F));
        *reinterpret_cast<bf16x4*>(map + map_px(b, y, x, F, C) + c) = vbg::to_bf16x4(ld4(feat + px * C + c));
    }
}

// ------------------------------------------------------------------------------------------- head tail
// conv5_{ctr,offset,size}: 1x1 conv W/8 -> 1 / 2 / 2 (+bias), then sigmoid + clamp on ctr and size
// (lib/models/layers/head.py:175-201).  t4: [3 towers][B * F * F][CW] (towers in the order ctr, offset, size), tower_stride elements
// between towers; w5: [5][CW] f32 rows = ctr, offset0, offset1, size0, size1;  b5: [5].  One thread per pixel, 16-byte loads.
// T: the element read -- bf16 (conv4's stored output) or float (conv4's f32 GEMM output before its ReLU: RELU applies it on the way in).
template <int CW, typename T, bool RELU>
__device__ __forceinline__ void conv5_body(const T* __restrict__ t4, const float* __restrict__ w5, const float* __restrict__ b5, int npix_total, int FF,
                                           size_t tower_stride, float* __restrict__ score, float* __restrict__ size, float* __restrict__ offset) {
    constexpr int VE = 16 / sizeof(T);
    typedef T vec __attribute__((ext_vector_type(VE)));
    __shared__ float sw[5 * CW + 5];
    for (int i = threadIdx.x; i < 5 * CW + 5; i += 256) sw[i] = i < 5 * CW ? w5[i] : b5[i - 5 * CW];
    __syncthreads();
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npix_total) return;
    float o[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) o[j] = sw[5 * CW + j];
#pragma unroll
    for (int tw = 0; tw < 3; ++tw) {
        const T* src = t4 + (size_t)tw * tower_stride + (size_t)p * CW;
#pragma unroll
        for (int cv = 0; cv < CW / VE; ++cv) {
            const vec v = *reinterpret_cast<const vec*>(src + cv * VE);
#pragma unroll
            for (int e = 0; e < VE; ++e) {
                const float a = RELU ? fmaxf((float)v[e], 0.f) : (float)v[e];
                const int c = cv * VE + e;
                if (tw == 0) o[0] = fmaf(a, sw[0 * CW + c], o[0]);
                if (tw == 1) { o[1] = fmaf(a, sw[1 * CW + c], o[1]); o[2] = fmaf(a, sw[2 * CW + c], o[2]); }
                if (tw == 2) { o[3] = fmaf(a, sw[3 * CW + c], o[3]); o[4] = fmaf(a, sw[4 * CW + c], o[4]); }
            }
        }
    }
    const int b = p / FF, px = p - b * FF;
    score[p] = sigmoid_clamped(o[0]);
    offset[((size_t)b * 2 + 0) * FF + px] = o[1];
    offset[((size_t)b * 2 + 1) * FF + px] = o[2];
    size[((size_t)b * 2 + 0) * FF + px] = sigmoid_clamped(o[3]);
    size[((size_t)b * 2 + 1) * FF + px] = sigmoid_clamped(o[4]);
}
template <int CW>
__global__ __launch_bounds__(256) void conv5_kernel(const bf16* __restrict__ t4, const float* __restrict__ w5,
                                                    const float* __restrict__ b5, int npix_total, int FF, size_t tower_stride,
                                                    float* __restrict__ score, float* __restrict__ size, float* __restrict__ offset) {
    conv5_body<CW, bf16, false>(t4, w5, b5, npix_total, FF, tower_stride, score, size, offset);
}

}  // namespace vbm

// vb_misc.h -- the HBM-bound kernels around the GEMMs of the ViT-Base path: patch gathering, LayerNorm, head tail.
#pragma once
#include "vb_gemm.h"
#include "vt_bf3.h"

namespace vbm {

using vbg::bf16;
using vbg::bf16x4;
using vbg::bf16x8;

// ---------------------------------------------------------------------------------------------- patches
// PatchEmbed's Conv2d(3, C, 16, stride 16) (lib/models/layers/patch_embed.py:20-32) as a GEMM: this kernel lays the
// crops out as its left operand P[m = frame * L + token][k = c * 256 + r * 16 + s] in bf16 (k order = the conv weight's
// own [3][16][16] order), template tokens first (combine_tokens 'direct', lib/models/ostrack/utils.py:13-14).
// One thread = 8 consecutive s of one (m, c, r): 32 B in, 16 B out, writes fully coalesced.
__global__ __launch_bounds__(256) void patchify_kernel(const float* __restrict__ z, const float* __restrict__ x,
                                                       bf16* __restrict__ P, int B, int Tz, int Tx) {
    const int gz = Tz / 16, gx = Tx / 16, Lz = gz * gz, L = Lz + gx * gx;
    const size_t total = (size_t)B * L * 96;                    // 96 = 3 * 16 * 2 chunks of 8 per patch
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int ch = (int)(i % 96);
        const size_t m = i / 96;
        const int t = (int)(m % L), f = (int)(m / L);
        const int c = ch >> 5, r = (ch >> 1) & 15, s0 = (ch & 1) * 8;
        const float* src;
        if (t < Lz) {
            const int py = t / gz, px = t - py * gz;
            src = z + (((size_t)f * 3 + c) * Tz + py * 16 + r) * Tz + px * 16 + s0;
        } else {
            const int tt = t - Lz, py = tt / gx, px = tt - py * gx;
            src = x + (((size_t)f * 3 + c) * Tx + py * 16 + r) * Tx + px * 16 + s0;
        }
        const bf16x4 lo = vbg::to_bf16x4(ld4(src)), hi = vbg::to_bf16x4(ld4(src + 4));
        *reinterpret_cast<bf16x8*>(P + m * 768 + ch * 8) = bf16x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    }
}

// The search rows of the same operand from the uint8 HWC patch (B, T, T, 3) that vt_crop_u8* writes (sample_target's output), DENSE:
// P[m = frame * (T / 16)^2 + token][k = c * 256 + r * 16 + s] = bf16(byte - centre).  Preprocessor.process's / 255, - mean, / std live in
// the weights this operand meets (vitb.hip fold_patch_u8); centre = 128 takes the bytes' common mode out of what those rounded weights
// multiply.  |byte - centre| has at most 8 significant bits: its bf16 is exact, the conversion is the float's upper half.
// One thread = pixel row r of one token: 48 contiguous bytes in (offset a multiple of 48: three aligned 16-byte loads), one 32-byte run out
// per channel.  r is the fastest lane index, so the 16 lanes of a token write each channel's 16 runs as ONE contiguous 512 bytes.
__global__ __launch_bounds__(256) void patchify_u8_kernel(const unsigned char* __restrict__ xp, bf16* __restrict__ P, int B, int T, float centre) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const int g = T / 16, Lx = g * g;
    const size_t total = (size_t)B * Lx * 16;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int r = (int)(i & 15);
        const size_t m = i >> 4;
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
            u32x4* dst = reinterpret_cast<u32x4*>(P + m * 768 + c * 256 + r * 16);
            dst[0] = u32x4{o[0], o[1], o[2], o[3]};
            dst[1] = u32x4{o[4], o[5], o[6], o[7]};
        }
    }
}

// -------------------------------------------------------------------------------------------- LayerNorm
// nn.LayerNorm(C, eps) over the f32 residual stream (lib/models/ostrack/vit.py:78,82,130; eps 1e-6): biased variance,
// two passes over registers.  One wave per token row, C = 768 = 64 lanes x 3 float4.
//   xn   (optional)  bf16 [M][C]                                   -> the next GEMM's left operand
//   map  (optional)  bf16 zero-bordered NHWC [B][F+2][F+2][C]: search rows only (forward_head's (B,C,F,F) view,
//                    lib/models/ostrack/ostrack.py:126-129)         -> the head's implicit-GEMM input
//   feat (optional)  f32 [B][Lx][C]: search rows only               -> stage API / tests
//   xb + rstd (optional, together)  the LayerNorm folded into the next GEMM (vb_gemm.h): bf16 copy of the RAW row and its
//                    1 / sqrt(var + eps) -- what the residual-writing GEMM epilogues + ln_finalize_kernel produce, for a
//                    residual stream that arrived from outside (vt_blocks on caller-supplied tokens)
template <int C>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ resid, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float eps, int M, int L, int Lz, int F,
                                                        bf16* __restrict__ xn, bf16* __restrict__ map, float* __restrict__ feat,
                                                        bf16* __restrict__ xb, float* __restrict__ rstd_out, float* __restrict__ mean_out) {
    static_assert(C % 256 == 0, "C = 64 lanes x float4 x n");
    constexpr int NV = C / 256;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* p = resid + (size_t)row * C;
    f4 v[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        v[i] = ld4(p + i * 256 + lane * 4);
        s += hsum4(v[i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s * (1.0f / C);
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        v[i] = v[i] - splat4(mean);
        ss += hsum4(v[i] * v[i]);
        // the raw rows' bf16 copy for the LayerNorm-folded GEMMs, CENTRED (vb_gemm.h Args::cm): the folded weights ignore a per-row constant
        if (xb) *reinterpret_cast<bf16x4*>(xb + (size_t)row * C + i * 256 + lane * 4) = vbg::to_bf16x4(v[i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    const float rstd = 1.0f / sqrtf(ss * (1.0f / C) + eps);
    if (rstd_out) {
        if (lane == 0) { rstd_out[row] = rstd; if (mean_out) mean_out[row] = mean; }
        if (!xn && !map && !feat) return;
    }
    const int f = row / L, t = row - f * L;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = i * 256 + lane * 4;
        const f4 y = v[i] * splat4(rstd) * ld4(gamma + c) + ld4(beta + c);
        if (xn) *reinterpret_cast<bf16x4*>(xn + (size_t)row * C + c) = vbg::to_bf16x4(y);
        if (t >= Lz) {
            const int tt = t - Lz;
            if (map) {
                const int yy = tt / F, xx = tt - yy * F, P = F + 2;
                *reinterpret_cast<bf16x4*>(map + ((size_t)(f * P + yy + 1) * P + xx + 1) * C + c) = vbg::to_bf16x4(y);
            }
            if (feat) st4(feat + ((size_t)f * (L - Lz) + tt) * C + c, y);
        }
    }
}

// The same LayerNorm at a width that is no multiple of 256 (ViT-Small 384, ViT-Tiny 192): C = 64 lanes x NV vectors of VW floats, VW = 2 at
// a multiple of 128, else 1 (C a multiple of 64).  All 64 lanes are active, so the butterfly sums no padding; a wave still reads and writes
// whole contiguous runs of 64 VW floats.  Its own kernel: layernorm_kernel<768 / 1024> keep their code.
template <int VW> struct LnVec;
template <> struct LnVec<1> { typedef float f; typedef bf16 b; };
template <> struct LnVec<2> { typedef vbg::f2 f; typedef vbg::bf16x2 b; };
template <int VW>
__device__ __forceinline__ float ln_hsum(typename LnVec<VW>::f v) {
    if constexpr (VW == 2) return v.x + v.y;
    else return v;
}
template <int VW>
__device__ __forceinline__ typename LnVec<VW>::b ln_to_bf16(typename LnVec<VW>::f v) {
    if constexpr (VW == 2) return __builtin_convertvector(v, vbg::bf16x2);
    else return (bf16)v;
}

template <int C>
__global__ __launch_bounds__(256) void layernorm_small_kernel(const float* __restrict__ resid, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps, int M, int L, int Lz, int F,
                                                              bf16* __restrict__ xn, bf16* __restrict__ map, float* __restrict__ feat,
                                                              bf16* __restrict__ xb, float* __restrict__ rstd_out, float* __restrict__ mean_out) {
    static_assert(C % 64 == 0 && C % 256 != 0, "C = 64 lanes x (float2 | float) x n; multiples of 256 take layernorm_kernel");
    constexpr int VW = C % 128 == 0 ? 2 : 1, NV = C / (64 * VW);
    typedef typename LnVec<VW>::f fv;
    typedef typename LnVec<VW>::b bv;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* p = resid + (size_t)row * C;
    fv v[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        v[i] = *reinterpret_cast<const fv*>(p + (i * 64 + lane) * VW);
        s += ln_hsum<VW>(v[i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s * (1.0f / C);
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        v[i] = v[i] - mean;
        ss += ln_hsum<VW>(v[i] * v[i]);
        if (xb) *reinterpret_cast<bv*>(xb + (size_t)row * C + (i * 64 + lane) * VW) = ln_to_bf16<VW>(v[i]);      // centred, as in layernorm_kernel
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    const float rstd = 1.0f / sqrtf(ss * (1.0f / C) + eps);
    if (rstd_out) {
        if (lane == 0) { rstd_out[row] = rstd; if (mean_out) mean_out[row] = mean; }
        if (!xn && !map && !feat) return;
    }
    const int f = row / L, t = row - f * L;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (i * 64 + lane) * VW;
        const fv y = v[i] * rstd * *reinterpret_cast<const fv*>(gamma + c) + *reinterpret_cast<const fv*>(beta + c);
        if (xn) *reinterpret_cast<bv*>(xn + (size_t)row * C + c) = ln_to_bf16<VW>(y);
        if (t >= Lz) {
            const int tt = t - Lz;
            if (map) {
                const int yy = tt / F, xx = tt - yy * F, P = F + 2;
                *reinterpret_cast<bv*>(map + ((size_t)(f * P + yy + 1) * P + xx + 1) * C + c) = ln_to_bf16<VW>(y);
            }
            if (feat) *reinterpret_cast<fv*>(feat + ((size_t)f * (L - Lz) + tt) * C + c) = y;
        }
    }
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
    static_assert(C % 4 == 0, "float4 lanes");
    constexpr int NV = (C + 255) / 256;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* p = resid + (size_t)row * C;
    f4 v[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = i * 256 + lane * 4;
        v[i] = c < C ? ld4(p + c) : splat4(0.f);
        s += hsum4(v[i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s * (1.0f / C);
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (i * 256 + lane * 4 < C) {
            v[i] = v[i] - splat4(mean);
            ss += hsum4(v[i] * v[i]);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    const float rstd = 1.0f / sqrtf(ss * (1.0f / C) + eps);
    const int f = row / L, t = row - f * L;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = i * 256 + lane * 4;
        if (c >= C) continue;
        const f4 y = v[i] * splat4(rstd) * ld4(gamma + c) + ld4(beta + c);
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
        const int x = (int)(px % F), y = (int)((px / F) % F), b = (int)(px / ((size_t)F * F)), P = F + 2;
        *reinterpret_cast<bf16x4*>(map + ((size_t)(b * P + y + 1) * P + x + 1) * C + c) = vbg::to_bf16x4(ld4(feat + px * C + c));
    }
}

// ------------------------------------------------------------------------------------------- head tail
// conv5_{ctr,offset,size}: 1x1 conv W/8 -> 1 / 2 / 2 (+bias), then sigmoid + clamp on ctr and size
// (lib/models/layers/head.py:175-201).  t4: [3 towers][B * F * F][CW] bf16 (towers in the order ctr, offset, size);
// w5: [5][CW] f32 rows = ctr, offset0, offset1, size0, size1;  b5: [5].  One thread per pixel.
template <int CW>
__global__ __launch_bounds__(256) void conv5_kernel(const bf16* __restrict__ t4, const float* __restrict__ w5,
                                                    const float* __restrict__ b5, int npix_total, int FF, size_t tower_stride,
                                                    float* __restrict__ score, float* __restrict__ size, float* __restrict__ offset) {
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
        const bf16* src = t4 + (size_t)tw * tower_stride + (size_t)p * CW;    // tower_stride: elements between towers
#pragma unroll
        for (int c8 = 0; c8 < CW / 8; ++c8) {
            const bf16x8 v = *reinterpret_cast<const bf16x8*>(src + c8 * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float a = (float)v[e];
                if (tw == 0) o[0] = fmaf(a, sw[0 * CW + c8 * 8 + e], o[0]);
                if (tw == 1) { o[1] = fmaf(a, sw[1 * CW + c8 * 8 + e], o[1]); o[2] = fmaf(a, sw[2 * CW + c8 * 8 + e], o[2]); }
                if (tw == 2) { o[3] = fmaf(a, sw[3 * CW + c8 * 8 + e], o[3]); o[4] = fmaf(a, sw[4 * CW + c8 * 8 + e], o[4]); }
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

}  // namespace vbm

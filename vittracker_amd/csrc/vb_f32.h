// vb_f32.h -- the fp32-equivalent mode of the patch-16 ViT path (vt_set_precision): what is not a GEMM.
//
// Every contraction of the mode is vbg::gemm_kernel on operands expanded to six bf16 k-ranges (vb_misc.h store_split8); activations between
// kernels are f32.  Here: the weight expansion, the patch operands (six terms from an fp32 crop, three from a uint8 patch: a byte is exact
// in one piece), the f32 attention, the head's map expansion and its 1 x 1 tail.
#pragma once
#include "vb_misc.h"

namespace vbf {

using vbg::bf16;

// ------------------------------------------------------------------------------------------------ weights
// w [rows][K] f32 -> [rows][terms x K] bf16: terms = 6: [wm | wl | wh | wm | wh | wh], the partner of store_split8's [xm | xh | xl | xh | xm | xh];
// terms = 3: [wl | wm | wh], against an operand that is exact in one piece, [b | b | b].  One thread = four columns.
__global__ __launch_bounds__(256) void expand_weight_kernel(const float* __restrict__ w, bf16* __restrict__ out, size_t rows, int K, int terms) {
    const size_t per = (size_t)K / 4, total = rows * per;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t r = i / per;
        const int c = (int)(i - r * per) * 4;
        vt3::u32x2 h, m, l;
        vbm::split3_rne(ld4(w + r * K + c), h, m, l);
        vt3::u32x2* p = reinterpret_cast<vt3::u32x2*>(out + r * terms * K + c);
        const int s = K / 4;
        if (terms == 6) { p[0] = m; p[s] = l; p[2 * s] = h; p[3 * s] = m; p[4 * s] = h; p[5 * s] = h; }
        else { p[0] = l; p[s] = m; p[2 * s] = h; }
    }
}

// ------------------------------------------------------------------------------------------------ patches
// vbm::patchify_kernel's dense form for one token kind, expanded: P[m = frame * (T / 16)^2 + token][6 x 768].  One thread = 8 consecutive s.
__global__ __launch_bounds__(256) void patchify_split_kernel(const float* __restrict__ img, bf16* __restrict__ P, int B, int T) {
    const int g = T / 16, Lk = g * g;
    const size_t total = (size_t)B * Lk * 96;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int ch = (int)(i % 96);
        const size_t m = i / 96;
        const int t = (int)(m % Lk), f = (int)(m / Lk);
        const float* src = vbm::crop_patch_src(img, T, g, f, t, ch);
        vbm::store_split8(P + m * (6 * 768), 768, ch * 8, ld4(src), ld4(src + 4));
    }
}

// vbm::patchify_u8_kernel's operand for the mode: P[m][3 x 768] = [b | b | b], b = bf16(byte) (exact, uncentred: the weights' three pieces
// carry Preprocessor.process to fp32 accuracy, so there is no rounding for a common mode to meet).  Same thread layout.
__global__ __launch_bounds__(256) void patchify_u8_split_kernel(const unsigned char* __restrict__ xp, bf16* __restrict__ P, int B, int T) {
    const int g = T / 16, Lx = g * g;
    const size_t total = (size_t)B * Lx * 16;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int r = (int)(i & 15);
        const size_t m = i >> 4;
        vbm::u8_row_unpack(xp, T, g, Lx, m, r, 0.f, [&](int c, vbg::u32x4 lo, vbg::u32x4 hi) {
#pragma unroll
            for (int seg = 0; seg < 3; ++seg) {
                vbg::u32x4* dst = reinterpret_cast<vbg::u32x4*>(P + m * (3 * 768) + seg * 768 + c * 256 + r * 16);
                dst[0] = lo;
                dst[1] = hi;
            }
        });
    }
}

// ---------------------------------------------------------------------------------------------- attention
// softmax(q k^T) v of one (frame, head, tile of AQ queries) per workgroup, on the f32 q | k | v rows [frame * L + token][3 C] the qkv GEMM
// leaves (q pre-scaled), in plain f32 FMAs.  lane = query, wave = a quarter of the keys: K and V go through LDS in chunks of AKC keys, and
// every LDS read of the inner loops is one address per wave (a broadcast: no bank conflict); a wave takes the chunk's sub-blocks of 8 keys
// w, w + 4, ... with an online maximum and sum per sub-block, and the four waves' (max, sum, o) are merged through LDS at the end.  L is a
// multiple of 8 (320, 720), so a sub-block is whole or absent -- the partial last chunk of 720 runs fewer sub-blocks, no masked key.
// Queries past L (the last tile of 720) compute on a clamped row and store nothing.  The output is written as the proj GEMM's expanded
// operand [M][6 C].  q is staged, and o merged, in rows of QS = 68 floats: lane-strided 16-byte LDS accesses then spread over all banks.
constexpr int AQ = 64, AKC = 64, AD = 64, QS = 68;
__global__ __launch_bounds__(256) void attn_f32_kernel(const float* __restrict__ qkv, bf16* __restrict__ out, int C, int heads, int L, int qtiles) {
    __shared__ __attribute__((aligned(16))) float sm[2 * AKC * AD];      // 32 KiB: K chunk | V chunk
    static_assert(AQ * QS + 2 * AQ <= 2 * AKC * AD, "the merge area fits the chunk area");
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int qt = blockIdx.x % qtiles, hh = (blockIdx.x / qtiles) % heads, f = blockIdx.x / (qtiles * heads);
    const int ldq = 3 * C, q0 = qt * AQ;
    const float* base = qkv + (size_t)f * L * ldq + hh * AD;
    const int sr = tid >> 4, c4 = (tid & 15) * 4;      // staging: 16 rows of 64 floats per pass
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int r = sr + 16 * p, qr = q0 + r < L ? q0 + r : L - 1;
        *reinterpret_cast<f4*>(sm + r * QS + c4) = ld4(base + (size_t)qr * ldq + c4);
    }
    __syncthreads();
    f4 q[16], o[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) { q[j] = *reinterpret_cast<const f4*>(sm + lane * QS + 4 * j); o[j] = splat4(0.f); }
    __syncthreads();
    float mx = -INFINITY, lsum = 0.f;
    float* const ks = sm;
    float* const vs = sm + AKC * AD;
    for (int k0 = 0; k0 < L; k0 += AKC) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int r = sr + 16 * p, kr = k0 + r < L ? k0 + r : L - 1;
            const float* src = base + (size_t)kr * ldq + c4;
            *reinterpret_cast<f4*>(ks + r * AD + c4) = ld4(src + C);
            *reinterpret_cast<f4*>(vs + r * AD + c4) = ld4(src + 2 * C);
        }
        __syncthreads();
        const int nk = L - k0 < AKC ? L - k0 : AKC;
        for (int sb = w; sb * 8 < nk; sb += 4) {
            float s[8];
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) {
                const float* kp = ks + (sb * 8 + kk) * AD;
                f4 a = splat4(0.f);
#pragma unroll
                for (int j = 0; j < 16; ++j) a = vbg::fma4(q[j], *reinterpret_cast<const f4*>(kp + 4 * j), a);
                s[kk] = hsum4(a);
            }
            float mn = mx;
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) mn = fmaxf(mn, s[kk]);
            const float corr = expf(mx - mn);      // (first sub-block: exp(-inf) = 0 on zeros)
            mx = mn;
            lsum *= corr;
#pragma unroll
            for (int j = 0; j < 16; ++j) o[j] = o[j] * splat4(corr);
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) {
                const float p = expf(s[kk] - mn);
                lsum += p;
                const float* vp = vs + (sb * 8 + kk) * AD;
#pragma unroll
                for (int j = 0; j < 16; ++j) o[j] = vbg::fma4(splat4(p), *reinterpret_cast<const f4*>(vp + 4 * j), o[j]);
            }
        }
        __syncthreads();
    }
    // merge: wave 0 writes its state, waves 1..3 fold theirs in, one after the other
    float* const om = sm;
    float* const mm = sm + AQ * QS;
    float* const lm = mm + AQ;
    for (int r = 0; r < 4; ++r) {
        if (w == r) {
            if (r == 0) {
#pragma unroll
                for (int j = 0; j < 16; ++j) *reinterpret_cast<f4*>(om + lane * QS + 4 * j) = o[j];
                mm[lane] = mx; lm[lane] = lsum;
            } else if (mx > -INFINITY) {      // (a wave that met no key has nothing to add)
                const float mo = mm[lane], mn = fmaxf(mo, mx), ca = expf(mo - mn), cb = expf(mx - mn);
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    f4* p = reinterpret_cast<f4*>(om + lane * QS + 4 * j);
                    *p = *p * splat4(ca) + o[j] * splat4(cb);
                }
                mm[lane] = mn; lm[lane] = lm[lane] * ca + lsum * cb;
            }
        }
        __syncthreads();
    }
    const int d8 = (tid & 7) * 8;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int r = (tid >> 3) + 32 * p;
        if (q0 + r >= L) continue;
        const float inv = 1.0f / lm[r];
        const f4 a = *reinterpret_cast<const f4*>(om + r * QS + d8) * splat4(inv), b = *reinterpret_cast<const f4*>(om + r * QS + d8 + 4) * splat4(inv);
        vbm::store_split8(out + ((size_t)f * L + q0 + r) * 6 * C, C, hh * AD + d8, a, b);
    }
}

// --------------------------------------------------------------------------------------------------- head
// f32 rows -> the zero-bordered map of expanded pixels [tower][frame][F+2][F+2][6 C] the A_CONV GEMM reads (channels per tap = 6 C: a pixel's
// six k-ranges; the conv weights are [cout][tap][6 cin]).  Source element (tower t = blockIdx.y, pixel p of the B frames, channel c) at
// src[t * src_tower + p * ld + c]: the search features (one tower, ld = C), a conv GEMM's f32 output (relu: its ReLU is applied here).
__global__ __launch_bounds__(256) void map_split_kernel(const float* __restrict__ src, size_t src_tower, int ld, bf16* __restrict__ dst, size_t dst_tower,
                                                        int B, int F, int C, int relu) {
    const size_t per = (size_t)C / 8, total = (size_t)B * F * F * per;
    src += blockIdx.y * src_tower;
    dst += blockIdx.y * dst_tower;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % per) * 8;
        const size_t px = i / per;
        const int x = (int)(px % F), y = (int)((px / F) % F), b = (int)(px / ((size_t)F * F));
        f4 u = ld4(src + px * ld + c), v = ld4(src + px * ld + c + 4);
        if (relu) {
            u = f4{fmaxf(u.x, 0.f), fmaxf(u.y, 0.f), fmaxf(u.z, 0.f), fmaxf(u.w, 0.f)};
            v = f4{fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)};
        }
        vbm::store_split8(dst + vbm::map_px(b, y, x, F, 6 * C), C, c, u, v);
    }
}

// vbm::conv5_kernel on conv4's f32 GEMM output t4 [3 towers][npix][CW] (before its ReLU, applied here)
template <int CW>
__global__ __launch_bounds__(256) void conv5_f32_kernel(const float* __restrict__ t4, const float* __restrict__ w5, const float* __restrict__ b5,
                                                        int npix_total, int FF, size_t tower_stride, float* __restrict__ score,
                                                        float* __restrict__ size, float* __restrict__ offset) {
    vbm::conv5_body<CW, float, true>(t4, w5, b5, npix_total, FF, tower_stride, score, size, offset);
}

}  // namespace vbf

// vt_track.h -- the steps either side of the network in Vit_dist.track(), on the device.
//
// crop_kernel replaces, per sequence, sample_target (lib/train/data/processing_utils.py:12-79:
// square crop of side ceil(sqrt(w*h)*factor) around the previous box, zero padding, cv.resize to
// T x T) followed by Preprocessor.process (lib/test/tracker/data_utils.py:11-17: /255, -mean, /std,
// HWC -> NCHW).  update_state_kernel replaces the tail of track() (lib/test/tracker/vit_dist.py:
// 107-111,150-156 and clip_box, lib/utils/box_ops.py:97-106).
//
// Numerics follow the reference's host code: box / crop geometry in double (Python floats),
// round-half-even for the crop origin (Python round()), OpenCV's INTER_LINEAR uint8 path in 11-bit
// fixed point (weights = round(w * 2048), horizontal pass in int, vertical pass
// (((b0*(S0>>4))>>16) + ((b1*(S1>>4))>>16) + 2) >> 2), float32 normalisation in the reference's
// operation order (as torch executes it on a GPU).  Integer stages are bit-exact against the host port in vittracker_amd/host_ops.py
// (which is itself unpinned against cv2: SURVEY.md 8(f) rank 1).
#pragma once
#include "vt_common.h"

namespace vtt {

struct CropGeom {     // per sequence, written by crop_kernel's first lane for update_state_kernel
    double resize_factor;   // T / crop_sz
};

// Source index and 11-bit weights of output coordinate d (OpenCV resize, linear, pixel centres).
__device__ __forceinline__ void lin_coeff(int d, int src, double scale, int& s0, int& s1, int& a0, int& a1) {
    float f = (float)((d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= src - 1) { s = src - 1; f = 0.f; }
    a1 = (int)rintf(f * 2048.f);
    a0 = (int)rintf((1.f - f) * 2048.f);
    s0 = s;
    s1 = s + 1 < src ? s + 1 : src - 1;
}

// ---- frame sources: where sequence b's frame lies.  A template parameter of the crop bodies below; each kernel form has a dense
// instantiation (today's (B,H,W,3) buffer with one H, W) and a frame-table twin (vt_crop_frames: one vt_frame per sequence).
struct FrameView {
    const unsigned char* base;     // the frame's first byte
    int H, W;
    unsigned pitch;                // bytes between rows
    unsigned nrec;                 // bytes readable from `base` (the buffer descriptor's bound: loads beyond it return zero, nothing is fetched)
    bool tail;                     // the frame's end may be the end of its allocation: crop_band_kernel guards the rows that reach it
    bool ok;                       // false: an unusable descriptor, poisoned like a too-small box
};
struct DenseFrames {      // frames (B,H,W,3): frame b at b H W 3; every frame's bound is the end of the batch, only the last one's is its own end
    static constexpr bool DENSE = true;
    __device__ __forceinline__ static FrameView view(const unsigned char* frames, int H, int W, int b, unsigned nb) {
        const size_t frame_bytes = (size_t)H * W * 3, rest = (size_t)(nb - b) * frame_bytes;      // bytes from this frame to the end of the batch
        return FrameView{frames + (size_t)b * frame_bytes, H, W, (unsigned)(W * 3), rest > 0xfffffff0ull ? 0xfffffff0u : (unsigned)rest,
                         b == (int)nb - 1, true};
    }
    // the frame's size alone (H, W, pitch, ok): what crop_band_kernel needs before its tables are built; the addresses come later, where
    // the dense form has always computed them (the dense instantiation keeps its registers)
    __device__ __forceinline__ static FrameView shape(const unsigned char*, int H, int W, int, unsigned) {
        return FrameView{nullptr, H, W, (unsigned)(W * 3), 0u, false, true};
    }
};
struct TableFrames {      // `frames` is a (B,) vt_frame table; H, W are unused
    static constexpr bool DENSE = false;
    __device__ __forceinline__ static FrameView view(const unsigned char* frames, int, int, int b, unsigned) {
        // one descriptor per workgroup at a workgroup-uniform address of a read-only argument: scalar LOADS into SGPRs, nothing else
        const vt_frame* const d = reinterpret_cast<const vt_frame*>(frames) + b;
        const unsigned char* const data = d->data;
        const int H = d->H, W = d->W;
        const long long pitch = d->pitch == 0 ? 3ll * W : d->pitch;
        // [data, data + pitch (H - 1) + 3 W) is the frame; it must be addressable by a 32-bit buffer offset
        const bool shape = H >= 1 && W >= 1 && W <= 0x10000000 && pitch >= 3ll * W && pitch <= 0xfffffff0ll;
        const unsigned long long ext = shape ? (unsigned long long)pitch * (unsigned long long)(H - 1) + 3ull * (unsigned long long)W : ~0ull;
        const bool ok = shape && data != nullptr && (reinterpret_cast<unsigned long long>(data) & 3ull) == 0 && ext <= 0xfffffff0ull;
        return FrameView{data, ok ? H : 1, ok ? W : 1, ok ? (unsigned)pitch : 3u, ok ? (unsigned)ext : 0u, true, ok};
    }
    __device__ __forceinline__ static FrameView shape(const unsigned char* frames, int H, int W, int b, unsigned nb) { return view(frames, H, W, b, nb); }
};

// ---- what every crop kernel below shares: the prologue of a workgroup (normalisation table, box geometry, poison), the table entries of
// a column and a row, and a band's guard row.  All forced inline: a kernel is still one function, and the measurements in the kernel
// comments below are of the kernels as wholes.
typedef unsigned u2v __attribute__((ext_vector_type(2)));
typedef unsigned u3v __attribute__((ext_vector_type(3)));
typedef unsigned u4v __attribute__((ext_vector_type(4)));
typedef unsigned u3a __attribute__((ext_vector_type(3), aligned(4)));      // a patch item's 12 bytes: 4-byte aligned only
typedef unsigned short us2 __attribute__((ext_vector_type(2)));

// Preprocessor.process maps a uint8 value to (v / 255 - mean) / std: 256 x 3 possible results.  They are computed ONCE per
// workgroup (256 threads, one value each) with the reference's arithmetic (three separately rounded fp32 ops, below) into an LDS
// table -- per output value one LDS read instead of a convert, a multiply, a subtract and an IEEE division sequence (~14 VALU
// instructions of the ~74 a value cost).  The caller's barrier publishes it.
__device__ __forceinline__ void fill_norm_lut(float* norm_lut, float m0, float m1, float m2, float s0, float s1, float s2) {
    const float meanv[3] = {m0, m1, m2}, stdq[3] = {s0, s1, s2};
    const int tid = threadIdx.x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        // torch's CUDA `tensor / 255.0` multiplies by the float reciprocal (div_true with a CPU scalar);
        // Preprocessor.process runs on the GPU, so that is the reference arithmetic
        // Three separately rounded ops, as three torch kernels: the empty asm keeps hipcc from
        // contracting the multiply and the subtraction into one fma (the _rn intrinsics do not).
        float scaled = (float)tid * (1.0f / 255.0f);
        asm volatile("" : "+v"(scaled));
        float centred = scaled - meanv[c];
        asm volatile("" : "+v"(centred));
        norm_lut[c * 256 + tid] = centred / stdq[c];
    }
}

// The square crop of sequence b in frame pixels (the fp64 geometry of sample_target) and what of it lies inside an H x W frame.
struct CropWindow {
    int crop_sz;                // side: ceil(sqrt(w h) factor); below 1: 'Too small bounding box.'
    int x1, y1;                 // origin, Python round(): half to even
    int vx0, vx1, vy0, vy1;     // valid source range of the padded crop
    double scale;               // crop_sz / T
};
__device__ __forceinline__ int crop_side(const double* states, int b, double factor) {
    return (int)ceil(sqrt(states[4 * b + 2] * states[4 * b + 3]) * factor);
}
__device__ __forceinline__ CropWindow crop_window(const double* states, int b, int crop_sz, int T, int H, int W) {      // crop_sz: crop_side's
    const double bx = states[4 * b + 0], by = states[4 * b + 1], bw = states[4 * b + 2], bh = states[4 * b + 3];
    const int x1 = (int)rint(bx + 0.5 * bw - crop_sz * 0.5);
    const int y1 = (int)rint(by + 0.5 * bh - crop_sz * 0.5);
    const int x2 = x1 + crop_sz, y2 = y1 + crop_sz;
    // the reference's pad formula keeps max(x2 - W + 1, 0) columns on the right, i.e. drops the last image column when the crop
    // reaches the border
    return CropWindow{crop_sz, x1, y1, x1 < 0 ? 0 : x1, x2 - (x2 - W + 1 > 0 ? x2 - W + 1 : 0), y1 < 0 ? 0 : y1, y2 - (y2 - H + 1 > 0 ? y2 - H + 1 : 0),
                      (double)crop_sz / (double)T};
}

// The reference raises 'Too small bounding box.' (processing_utils.py:33-34) where crop_sz < 1.  A kernel cannot raise: the crop and
// its resize factor are poisoned with NaN, so every box derived from them is NaN and the caller sees it (BatchedVitTracker checks
// user-supplied boxes on the host before they get here; boxes produced by vt_update_state are at least `margin` wide and never take
// this branch).  An unusable frame or image descriptor is poisoned the same way.  Patch bytes cannot carry the poison and are zeroed:
// the NaN resize factor carries it.  poison_item writes the item at (oy, ox0 .. ox0 + 3); RAGGED: T may be no multiple of 4.
template <bool U8OUT, bool RAGGED>
__device__ __forceinline__ void poison_item(float* out, unsigned char* out8, int b, int T, int oy, int ox0) {
    if constexpr (RAGGED) {
        for (int c = 0; c < 3; ++c)
            for (int k = 0; k < 4 && ox0 + k < T; ++k) {
                if constexpr (U8OUT) out8[((size_t)oy * T + ox0 + k) * 3 + c] = 0;
                else out[(((size_t)b * 3 + c) * T + oy) * T + ox0 + k] = __builtin_nanf("");
            }
    } else {
        if constexpr (U8OUT) *reinterpret_cast<u3a*>(out8 + ((size_t)oy * T + ox0) * 3) = u3a{0u, 0u, 0u};
        else {
            float* const o = out + (((size_t)b * 3) * T + oy) * T + ox0;
            for (int c = 0; c < 3; ++c) st4(o + (size_t)c * T * T, splat4(__builtin_nanf("")));
        }
    }
}
// ... and a band's IPT items of this thread (column group cg, rows row0 + j RPG + rl), with the sequence's resize factor
template <bool U8OUT, int T, int IPT, int RPG>
__device__ __forceinline__ void poison_band(float* out, unsigned char* out8, double* resize_factor, int b, int row0, int rl, int cg) {
    if (blockIdx.x == 0 && threadIdx.x == 0) resize_factor[b] = __builtin_nan("");
#pragma unroll
    for (int j = 0; j < IPT; ++j) poison_item<U8OUT, false>(out, out8, b, T, row0 + j * RPG + rl, 4 * cg);
}

// Output column ox: its two source columns in the frame, whether each lies inside the valid range (outside: zero padding), their
// 11-bit weights, and the base pixel xb of the pair's window: the left column when it is inside the frame, else the right one (then
// the left is padding)
struct ColumnTap { int xx0, xx1, xb, ax0, ax1; bool vc0, vc1; };
__device__ __forceinline__ ColumnTap column_tap(int ox, const CropWindow& g) {
    int sx0, sx1, ax0, ax1;
    lin_coeff(ox, g.crop_sz, g.scale, sx0, sx1, ax0, ax1);
    const int xx0 = g.x1 + sx0, xx1 = g.x1 + sx1;
    const bool vc0 = xx0 >= g.vx0 && xx0 < g.vx1, vc1 = xx1 >= g.vx0 && xx1 < g.vx1;
    return ColumnTap{xx0, xx1, vc0 ? xx0 : (vc1 ? xx1 : 0), ax0, ax1, vc0, vc1};
}
// the xtab entries of the table-driven kernels: zero padding lives in the WEIGHTS (packed for v_dot2: a padded column weighs nothing).
// RGB frames: window byte offset, weights, the right column's bit offset inside the window (0 or 24), -
__device__ __forceinline__ u4v frame_column_entry(const ColumnTap& t) {
    return u4v{3u * (unsigned)t.xb, (unsigned)(t.vc0 ? t.ax0 : 0) | ((unsigned)(t.vc1 ? t.ax1 : 0) << 16), (unsigned)(t.vc1 ? 24 * (t.xx1 - t.xb) : 0), 0u};
}
// vt_image layouts: plane-0 byte offset of the left tap (bpp bytes a pixel, yadd: see yuv_layout), weights, steps (bit 0 = the right
// tap is the next pixel, bit 1 = its chroma pair is the next pair), chroma byte offset (cmul bytes a pair; cxs: a pair is 1 << cxs
// pixels wide -- 1, or 0 where every pixel has its own chroma)
__device__ __forceinline__ u4v image_column_entry(const ColumnTap& t, unsigned bpp, unsigned yadd, unsigned cmul, unsigned cxs = 1u) {
    const unsigned step = t.vc1 && t.xx1 != t.xb ? 1u : 0u, cstep = t.vc1 && (t.xx1 >> cxs) != (t.xb >> cxs) ? 2u : 0u;
    return u4v{bpp * (unsigned)t.xb + yadd, (unsigned)(t.vc0 ? t.ax0 : 0) | ((unsigned)(t.vc1 ? t.ax1 : 0) << 16), step | cstep, cmul * ((unsigned)t.xb >> cxs)};
}

// Output row oy: its two source rows (a row outside the valid range reads row 0), their 11-bit weights and validity
struct RowTap {
    unsigned ya, yb;
    int by0, by1;
    bool vr0, vr1;
    __device__ __forceinline__ unsigned w0() const { return vr0 ? (unsigned)by0 << 12 : 0u; }      // << 12 for mulhi24; a padded row weighs nothing
    __device__ __forceinline__ unsigned w1() const { return vr1 ? (unsigned)by1 << 12 : 0u; }
};
__device__ __forceinline__ RowTap row_tap(int oy, const CropWindow& g) {
    int sy0, sy1, by0, by1;
    lin_coeff(oy, g.crop_sz, g.scale, sy0, sy1, by0, by1);
    const int yy0 = g.y1 + sy0, yy1 = g.y1 + sy1;
    const bool vr0 = yy0 >= g.vy0 && yy0 < g.vy1, vr1 = yy1 >= g.vy0 && yy1 < g.vy1;
    return RowTap{(unsigned)(vr0 ? yy0 : 0), (unsigned)(vr1 ? yy1 : 0), by0, by1, vr0, vr1};
}
// A band's tables, before its barrier.  xtab: the first T threads, one column each (`column`: the entry of a ColumnTap).  ytab, by the
// LAST NROWS threads (the first T are busy with the columns), per output row of the band: byte offsets of its two source rows in plane
// 0, their weights << 12.  ctab (may be null), per output row: the chroma-row offsets (y >> cys) cpitch of its two source rows.
template <int T, int NROWS, class Column>
__device__ __forceinline__ void fill_band_tables(unsigned* xtab, unsigned* ytab, unsigned* ctab, int row0, const CropWindow& g,
                                                 unsigned pitch0, unsigned cys, unsigned cpitch, Column&& column) {
    const int tid = threadIdx.x;
    if (tid < T) *reinterpret_cast<u4v*>(xtab + 4 * tid) = column(column_tap(tid, g));
    if (tid >= 256 - NROWS) {
        const int r = tid - (256 - NROWS);
        const RowTap t = row_tap(row0 + r, g);
        *reinterpret_cast<u4v*>(ytab + 4 * r) = u4v{t.ya * pitch0, t.yb * pitch0, t.w0(), t.w1()};
        if (ctab != nullptr) *reinterpret_cast<u2v*>(ctab + 2 * r) = u2v{(t.ya >> cys) * cpitch, (t.yb >> cys) * cpitch};
    }
}
// the last source row a band's guards have to reckon with: the lower tap of its last output row (rows beyond the valid range read row 0)
template <int NROWS>
__device__ __forceinline__ int band_last_source_row(int row0, const CropWindow& g) {
    int sl0, sl1, al0, al1;
    lin_coeff(row0 + NROWS - 1, g.crop_sz, g.scale, sl0, sl1, al0, al1);
    return g.y1 + sl1 < g.vy1 - 1 ? g.y1 + sl1 : g.vy1 - 1;
}

// grid (ceil(T * ceil(T/4) / 256), B); frames (B,H,W,3) uint8; states (B,4) double [x,y,w,h]; out (B,3,T,T) float.
// One thread = four consecutive output pixels of a row (all three channels): the vertical coefficients are computed once,
// and a channel's four values leave as ONE 16-byte store when T is a multiple of 4 (the crop sizes the tracker uses are:
// 64 / 128 / 256), i.e. whole 256-byte row segments per quarter-wave instead of 4-byte stores.
// BYTES = true: the same kernel with every 8-byte window assembled from eight single-byte loads -- the form that needs nothing of the
// device's unaligned-access mode; vt_create's self test (vittrack.hip: crop_selftest) selects it when the fast form's result differs.
// U8OUT (round 6): `out` is the uint8 (B, T, T, 3) patch itself -- sample_target's return value, before Preprocessor.process -- which
// the stems' uint8 forms consume (vt_stem.h: L1In); no normalisation table, a thread's 12 values leave as one 12-byte store.
// Src: the frame source (DenseFrames: crop_kernel; TableFrames: crop_frames_kernel).
template <class Src, bool BYTES, bool U8OUT>
__device__ __forceinline__ void crop_body(const unsigned char* __restrict__ frames, int H, int W,
                                          const double* __restrict__ states, double factor, int T,
                                          float m0, float m1, float m2, float s0, float s1, float s2,
                                          float* __restrict__ out, double* __restrict__ resize_factor) {
    const int b = blockIdx.y;
    const FrameView fv = Src::view(frames, H, W, b, gridDim.y);
    __shared__ float norm_lut[U8OUT ? 1 : 3 * 256];
    if constexpr (!U8OUT) {
        fill_norm_lut(norm_lut, m0, m1, m2, s0, s1, s2);
        __syncthreads();
    }
    unsigned char* const out8 = reinterpret_cast<unsigned char*>(out) + (size_t)b * T * T * 3;      // U8OUT: this frame's patch
    const int crop_sz = crop_side(states, b, factor);
    const int T4 = (T + 3) >> 2;                      // pixel groups per row
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (!(crop_sz >= 1) || !fv.ok) {
        if (idx == 0) resize_factor[b] = __builtin_nan("");
        if (idx < T * T4) poison_item<U8OUT, true>(out, out8, b, T, idx / T4, (idx - idx / T4 * T4) * 4);
        return;
    }
    const CropWindow g = crop_window(states, b, crop_sz, T, fv.H, fv.W);
    if (idx == 0) resize_factor[b] = (double)T / (double)crop_sz;
    if (idx >= T * T4) return;
    const int oy = idx / T4, ox0 = (idx - oy * T4) * 4;
    // a thread's own row and columns, with validity masks (not row_tap / column_tap: through them crop_kernel<false, *> takes 52 / 53 VGPRs for 51 / 52)
    int sy0, sy1, by0, by1;
    lin_coeff(oy, g.crop_sz, g.scale, sy0, sy1, by0, by1);
    // Source pixels: an RGB pixel is 3 consecutive bytes, and the two columns a bilinear sample reads are neighbours (or the same
    // pixel at the crop's edge), so ONE 8-byte load at byte offset 3 x covers both -- 8 loads per thread instead of 48 single-byte
    // loads, which were the kernel's cost (3072 vector-memory instructions per 128 x 128 crop: 33 us at batch 256, a quarter of the
    // tracker step).  Buffer loads at byte-unaligned offsets (tools/src/probe_unaligned.hip: the hardware returns the right bytes;
    // a load that crosses the end of the buffer returns zeros, so the frame's last pixels are read 8 bytes back and shifted).
    const unsigned nrec = fv.nrec;      // dense: bytes from this frame to the end of the batch; table: the frame's own extent
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(fv.base), 0, (int)nrec, 0x00020000);
    const int yy0 = g.y1 + sy0, yy1 = g.y1 + sy1;
    const bool vr0 = yy0 >= g.vy0 && yy0 < g.vy1, vr1 = yy1 >= g.vy0 && yy1 < g.vy1;
    const unsigned rowo0 = (unsigned)(vr0 ? yy0 : 0) * fv.pitch, rowo1 = (unsigned)(vr1 ? yy1 : 0) * fv.pitch;
    auto load8 = [&](unsigned off) -> unsigned long long {      // bytes off .. off + 7 of the frame (the last bytes of the batch: shifted in)
        if constexpr (BYTES) {
            unsigned long long r = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j)       // out-of-range bytes read as zero (buffer bounds), as in the fast form after its shift
                r |= (unsigned long long)(__builtin_amdgcn_raw_buffer_load_b8(rsrc, (int)(off + j), 0, 0) & 0xffu) << (8 * j);
            return r;
        }
        const unsigned over = off + 8u > nrec ? off + 8u - nrec : 0u;
        const u2v v = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)(off - over), 0, 0);
        return (((unsigned long long)v.y << 32) | v.x) >> (8u * over);
    };
    float res[3][4];
    unsigned pk[3] = {0u, 0u, 0u};      // U8OUT: the 12 bytes of this thread's four pixels, HWC
    unsigned long long q0[4], q1[4];
    int ax0a[4], ax1a[4], sh1[4];
    bool vc0a[4], vc1a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {       // all eight loads first
        const int ox = ox0 + k < T ? ox0 + k : T - 1;
        int sx0, sx1;
        lin_coeff(ox, g.crop_sz, g.scale, sx0, sx1, ax0a[k], ax1a[k]);
        const int xx0 = g.x1 + sx0, xx1 = g.x1 + sx1;
        vc0a[k] = xx0 >= g.vx0 && xx0 < g.vx1; vc1a[k] = xx1 >= g.vx0 && xx1 < g.vx1;
        // base pixel of the 8-byte window: the left column when it is inside the frame, else the right one (then the left is padding)
        const int xb = vc0a[k] ? xx0 : (vc1a[k] ? xx1 : 0);
        sh1[k] = vc1a[k] ? 24 * (xx1 - xb) : 0;                     // bit offset of the right column's pixel inside the window: 0 or 24
        q0[k] = load8(rowo0 + 3u * (unsigned)xb);
        q1[k] = load8(rowo1 + 3u * (unsigned)xb);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ax0 = ax0a[k], ax1 = ax1a[k];
        const bool vc0 = vc0a[k], vc1 = vc1a[k];
        // the left column is at bit 0 of the window when it is valid (it is the base); the right one at sh1 (0 when it is the base itself)
        // pixel (cy, cx) of the zero-padded crop: the frame inside the valid range, 0 outside (masked once per pixel, all channels)
        const unsigned l0 = vr0 && vc0 ? (unsigned)q0[k] : 0u, l1 = vr1 && vc0 ? (unsigned)q1[k] : 0u;
        const unsigned r0w = vr0 && vc1 ? (unsigned)(q0[k] >> sh1[k]) : 0u, r1w = vr1 && vc1 ? (unsigned)(q1[k] >> sh1[k]) : 0u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            // item 7b: not merged, see NOTES.md (crop kernels)
            const int p00 = (int)((l0 >> (8 * c)) & 0xffu), p01 = (int)((r0w >> (8 * c)) & 0xffu);
            const int p10 = (int)((l1 >> (8 * c)) & 0xffu), p11 = (int)((r1w >> (8 * c)) & 0xffu);
            // every factor is below 2^24 (8-bit pixels, 12-bit weights, 15-bit row sums): the 24-bit multiplier gives the same integers
            const int r0 = __mul24(p00, ax0) + __mul24(p01, ax1);
            const int r1 = __mul24(p10, ax0) + __mul24(p11, ax1);
            int v = ((__mul24(by0, r0 >> 4) >> 16) + (__mul24(by1, r1 >> 4) >> 16) + 2) >> 2;
            v = v < 0 ? 0 : (v > 255 ? 255 : v);
            if constexpr (U8OUT) pk[(3 * k + c) >> 2] |= (unsigned)v << (8 * ((3 * k + c) & 3));
            else res[c][k] = norm_lut[c * 256 + v];
        }
    }
    if constexpr (U8OUT) {
        unsigned char* o = out8 + ((size_t)oy * T + ox0) * 3;
        if ((T & 3) == 0) {
            typedef unsigned u3a __attribute__((ext_vector_type(3), aligned(4)));
            *reinterpret_cast<u3a*>(o) = u3a{pk[0], pk[1], pk[2]};
        } else {
            for (int i = 0; i < 12 && ox0 + i / 3 < T; ++i) o[i] = (unsigned char)(pk[i >> 2] >> (8 * (i & 3)));
        }
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float* o = out + (((size_t)b * 3 + c) * T + oy) * T + ox0;
        if ((T & 3) == 0) {
            st4(o, f4{res[c][0], res[c][1], res[c][2], res[c][3]});
        } else {
            for (int k = 0; k < 4 && ox0 + k < T; ++k) o[k] = res[c][k];
        }
    }
}
template <bool BYTES = false, bool U8OUT = false>
__global__ __launch_bounds__(256) void crop_kernel(const unsigned char* __restrict__ frames, int H, int W,
                                                   const double* __restrict__ states, double factor, int T,
                                                   float m0, float m1, float m2, float s0, float s1, float s2,
                                                   float* __restrict__ out, double* __restrict__ resize_factor) {
    crop_body<DenseFrames, BYTES, U8OUT>(frames, H, W, states, factor, T, m0, m1, m2, s0, s1, s2, out, resize_factor);
}
// the frame-table twin (vt_crop_frames): `frames` is a (B,) vt_frame table, H / W unused
template <bool BYTES = false, bool U8OUT = false>
__global__ __launch_bounds__(256) void crop_frames_kernel(const unsigned char* __restrict__ frames, int H, int W,
                                                          const double* __restrict__ states, double factor, int T,
                                                          float m0, float m1, float m2, float s0, float s1, float s2,
                                                          float* __restrict__ out, double* __restrict__ resize_factor) {
    crop_body<TableFrames, BYTES, U8OUT>(frames, H, W, states, factor, T, m0, m1, m2, s0, s1, s2, out, resize_factor);
}

// The crop as the tracker's step runs it (T a multiple of 4, T <= CROP_FAST_MAX_T): same arithmetic, same results bit for bit as
// crop_kernel (which stays: any T, the byte-load form, the reference of the device self test).  What differs:
//   - a workgroup computes the T column entries of its frame ONCE into LDS (byte offset of the 8-byte window, the two 11-bit weights
//     packed for v_dot2, the right column's bit offset) and walks G groups of 256 items (an item = four consecutive pixels of a row):
//     the column table, the normalisation table and the fp64 box geometry are paid once per G x 12 output values of a thread
//   - the walk is software-pipelined (group g + 1's eight window loads are issued before group g's arithmetic).  MEASURED (256 sequences,
//     rocprofv3 of tracking/track_batch_demo.py, us per launch at G128 / G256; crop_kernel: 25.1 / 111.3): G = 1: 22.3 / 106.3,
//     G = 2: 22.6 / 129.0, G = 4: 26.1 / 126.5 -- one item per thread stays the best shape, so G = 1 is what launch_crop uses;
//     windows fetched as three ALIGNED dwords + funnel shift (half the address-path cycles by tools/src/probe_gather.hip): 26.2 / 111.5
//     at G = 1, i.e. slower, and removed again.  The kernel is bound by neither its instruction count (a third of crop_kernel's in
//     the arithmetic) nor the gather's address path alone; NOTES R5-8.
//   - zero padding lives in the WEIGHTS: a column / row of the padded crop outside the frame gets weight 0, so the arithmetic carries
//     no validity masks
//   - the horizontal pass of a (row, channel) is v_perm_b32 (the channel's byte of the left and the right pixel into the two halves
//     of a dword) + v_dot2_u32_u16 with the packed weights; the vertical pass's (b (r >> 4)) >> 16 is one v_mul_hi_u32_u24
//   - a load that could cross the end of the buffer (the last rows of the last frame) shifts its window as crop_kernel does, on a
//     slow path a whole wave takes or skips
constexpr int CROP_FAST_MAX_T = 512;
#ifndef VT_CROPF_DBG
#define VT_CROPF_DBG 0      // timing builds only (wrong results): 1 = no frame loads, 2 = no stores, 4 = every workgroup reads frame 0, 8 = no arithmetic
#endif
__device__ __forceinline__ unsigned mulhi24(unsigned a, unsigned b) {      // (a b) >> 32 for a, b < 2^24
    unsigned r;
    asm("v_mul_hi_u32_u24 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// dst's byte N = (v >> 2) & 0xff, its other bytes kept: the vertical pass's final shift written straight into the packed patch bytes
// (SDWA destination select; `two` = a register holding 2)
__device__ __forceinline__ void put_byte_shr2(unsigned& dst, unsigned v, unsigned two, int n) {      // n: a constant once the callers' loops are unrolled
    switch (n) {
        case 0: asm("v_lshrrev_b32_sdwa %0, %1, %2 dst_sel:BYTE_0 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(dst) : "v"(two), "v"(v)); break;
        case 1: asm("v_lshrrev_b32_sdwa %0, %1, %2 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(dst) : "v"(two), "v"(v)); break;
        case 2: asm("v_lshrrev_b32_sdwa %0, %1, %2 dst_sel:BYTE_2 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(dst) : "v"(two), "v"(v)); break;
        default: asm("v_lshrrev_b32_sdwa %0, %1, %2 dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(dst) : "v"(two), "v"(v)); break;
    }
}
template <class Src, int G, bool U8OUT>
__device__ __forceinline__ void crop_fast_body(const unsigned char* __restrict__ frames, int H, int W,
                                               const double* __restrict__ states, double factor, int T,
                                               float m0, float m1, float m2, float s0, float s1, float s2,
                                               float* __restrict__ out, double* __restrict__ resize_factor) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const FrameView fv = Src::view(frames, H, W, b, gridDim.y);
    __shared__ float norm_lut[U8OUT ? 1 : 3 * 256];
    __shared__ __attribute__((aligned(16))) unsigned xtab[CROP_FAST_MAX_T * 4];      // per output column: window byte offset, weights, right column's shift, -
    unsigned char* const out8 = reinterpret_cast<unsigned char*>(out) + (size_t)b * T * T * 3;      // U8OUT: this frame's (T, T, 3) patch
    if constexpr (!U8OUT) fill_norm_lut(norm_lut, m0, m1, m2, s0, s1, s2);
    const int crop_sz = crop_side(states, b, factor);
    const int T4 = T >> 2, nitems = T * T4;
    const int item0 = blockIdx.x * G * 256;
    if (!(crop_sz >= 1) || !fv.ok) {
        if (blockIdx.x == 0 && tid == 0) resize_factor[b] = __builtin_nan("");
        for (int gi = 0; gi < G; ++gi) {
            const int idx = item0 + gi * 256 + tid;
            if (idx < nitems) poison_item<U8OUT, false>(out, out8, b, T, idx / T4, (idx - idx / T4 * T4) * 4);
        }
        return;
    }
    const CropWindow g = crop_window(states, b, crop_sz, T, fv.H, fv.W);
    if (blockIdx.x == 0 && tid == 0) resize_factor[b] = (double)T / (double)crop_sz;
    for (int ox = tid; ox < T; ox += 256) *reinterpret_cast<u4v*>(xtab + 4 * ox) = frame_column_entry(column_tap(ox, g));
    __syncthreads();
    const unsigned nrec = fv.nrec;
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(((VT_CROPF_DBG & 4) && Src::DENSE) ? frames : fv.base), 0, (int)nrec, 0x00020000);
    struct Item {
        unsigned long long q0[4], q1[4];
        unsigned wp[4], sh[4], byw0, byw1;
        int oy, ox0;
        bool live;
    };
    auto fetch = [&](int gi, Item& it) {
        const int idx = item0 + gi * 256 + tid;
        it.live = idx < nitems;
        const int idc = it.live ? idx : nitems - 1;
        it.oy = idc / T4;
        it.ox0 = (idc - it.oy * T4) * 4;
        const RowTap rt = row_tap(it.oy, g);
        const unsigned rowo0 = rt.ya * fv.pitch, rowo1 = rt.yb * fv.pitch;
        it.byw0 = rt.w0();
        it.byw1 = rt.w1();
        // can a window of this item cross the end of the buffer?  (3 (W - 1) is the largest column offset)
        const unsigned far = (rowo0 > rowo1 ? rowo0 : rowo1) + 3u * (unsigned)(fv.W - 1) + 8u;
        const bool slow = __builtin_amdgcn_ballot_w64(far > nrec) != 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const u4v e = *reinterpret_cast<const u4v*>(xtab + 4 * (it.ox0 + k));
            it.wp[k] = e.y; it.sh[k] = e.z;
            const unsigned o0 = rowo0 + e.x, o1 = rowo1 + e.x;
            if (VT_CROPF_DBG & 1) {
                it.q0[k] = ((unsigned long long)o0 << 32) | o1;
                it.q1[k] = ((unsigned long long)o1 << 32) | o0;
            } else
            if (slow) {
                const unsigned ov0 = o0 + 8u > nrec ? o0 + 8u - nrec : 0u, ov1 = o1 + 8u > nrec ? o1 + 8u - nrec : 0u;
                const u2v a = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)(o0 - ov0), 0, 0);
                const u2v c = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)(o1 - ov1), 0, 0);
                it.q0[k] = (((unsigned long long)a.y << 32) | a.x) >> (8u * ov0);
                it.q1[k] = (((unsigned long long)c.y << 32) | c.x) >> (8u * ov1);
            } else {
                const u2v a = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)o0, 0, 0);
                const u2v c = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)o1, 0, 0);
                it.q0[k] = ((unsigned long long)a.y << 32) | a.x;
                it.q1[k] = ((unsigned long long)c.y << 32) | c.x;
            }
        }
    };
    // item 7: not merged, see NOTES.md (crop kernels)
    auto finish = [&](const Item& it) {
        float res[3][4];
        unsigned pk[3] = {0u, 0u, 0u};      // U8OUT: the 12 bytes of the item's four pixels, HWC
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned l0 = (unsigned)it.q0[k], l1 = (unsigned)it.q1[k];
            const unsigned r0w = __builtin_amdgcn_alignbit((unsigned)(it.q0[k] >> 32), l0, it.sh[k]);       // the window >> 0 or 24 bits
            const unsigned r1w = __builtin_amdgcn_alignbit((unsigned)(it.q1[k] >> 32), l1, it.sh[k]);
            const us2 wv = __builtin_bit_cast(us2, it.wp[k]);
            if ((VT_CROPF_DBG & 8) && U8OUT) { pk[k % 3] ^= l0 ^ l1 ^ r0w ^ r1w ^ it.wp[k]; continue; }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                // bytes of the result: [left pixel's channel c, 0, right pixel's channel c, 0]
                const unsigned sel = 0x0c040c00u + 0x00010001u * (unsigned)c;
                const unsigned r0 = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, __builtin_amdgcn_perm(r0w, l0, sel)), wv, 0u, false);
                const unsigned r1 = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, __builtin_amdgcn_perm(r1w, l1, sel)), wv, 0u, false);
                // (b (r >> 4)) >> 16 = ((b << 12) (r with its low 4 bits cleared)) >> 32: one 24-bit high multiply (both factors < 2^24)
                const unsigned t0 = mulhi24(it.byw0, r0 & ~15u), t1 = mulhi24(it.byw1, r1 & ~15u);
                // v = (t0 + t1 + 2) >> 2, clamped at 255; its table entry is at byte 4 v
                if constexpr (U8OUT) {
                    unsigned v = (t0 + t1 + 2u) >> 2;
                    v = v > 255u ? 255u : v;
                    pk[(3 * k + c) >> 2] |= v << (8 * ((3 * k + c) & 3));
                } else {
                unsigned v4 = (t0 + t1 + 2u) & ~3u;
                v4 = v4 > 1020u ? 1020u : v4;
                res[c][k] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(norm_lut) + c * 1024 + v4);
                }
            }
        }
        if constexpr (U8OUT) {
            if ((VT_CROPF_DBG & 2) ? (pk[0] == 0x12345678u && pk[1] == 0x9abcdef0u) : it.live) *reinterpret_cast<u3a*>(out8 + ((size_t)it.oy * T + it.ox0) * 3) = u3a{pk[0], pk[1], pk[2]};
        } else
        if (it.live) {
#pragma unroll
            for (int c = 0; c < 3; ++c) st4(out + (((size_t)b * 3 + c) * T + it.oy) * T + it.ox0, f4{res[c][0], res[c][1], res[c][2], res[c][3]});
        }
    };
    Item buf[2];
    fetch(0, buf[0]);
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
        if (gi + 1 < G) fetch(gi + 1, buf[(gi + 1) & 1]);
        finish(buf[gi & 1]);
    }
}
template <int G, bool U8OUT = false>
__global__ __launch_bounds__(256) void crop_fast_kernel(const unsigned char* __restrict__ frames, int H, int W,
                                                        const double* __restrict__ states, double factor, int T,
                                                        float m0, float m1, float m2, float s0, float s1, float s2,
                                                        float* __restrict__ out, double* __restrict__ resize_factor) {
    crop_fast_body<DenseFrames, G, U8OUT>(frames, H, W, states, factor, T, m0, m1, m2, s0, s1, s2, out, resize_factor);
}
template <int G, bool U8OUT = false>      // the frame-table twin
__global__ __launch_bounds__(256) void crop_fast_frames_kernel(const unsigned char* __restrict__ frames, int H, int W,
                                                               const double* __restrict__ states, double factor, int T,
                                                               float m0, float m1, float m2, float s0, float s1, float s2,
                                                               float* __restrict__ out, double* __restrict__ resize_factor) {
    crop_fast_body<TableFrames, G, U8OUT>(frames, H, W, states, factor, T, m0, m1, m2, s0, s1, s2, out, resize_factor);
}

// crop_band_kernel (round 6) -- the crop at the tracker's sizes (T = 64 / 128 / 256: T / 4 = 2^LGT4 column groups), same arithmetic and
// results bit for bit as crop_fast_kernel / crop_kernel.  Measured on timing builds of crop_fast_kernel (tools/crop_ab.py, T = 128, 256
// frames, us per launch alone): everything 13.8 * no frame loads 11.6 * no loads and no stores 9.3 * no arithmetic 12.9; T = 256: 39.2 for
// 4 x the items -- the kernel is bound by the vector instructions it issues (~500 per item of 12 values, of which the fp64 box geometry,
// the column entry, the row coefficients and the index arithmetic every thread repeats are ~210), not by its traffic.  Here a workgroup
// owns a BAND of IPT x 256 items and a thread IPT items of ONE column group:
//   - geometry, the column table and the band's row table (row byte offsets + vertical weights, one entry per output row) are computed
//     once per IPT x 256 items; a thread reads its four column entries into registers once and one row entry per item
//   - the IPT x 8 window loads of a thread are all in flight before the first item's arithmetic (what a thread per item had in flight
//     as IPT threads), instead of crop_fast_kernel<G>'s two-deep software pipeline, which halved the loads in flight and lost (NOTES R5-8)
//   - only the LAST frame of the batch can read past the buffer's end: the shifted-window slow path is a workgroup-uniform branch
//   - ALIGNED: stamps (tools/crop_stamps.py, -DVT_CROPF_DBG=16) put 12.3 k of a band's 16.6 k cycles into ISSUING its 32 window loads per
//     thread: a byte-aligned 8-byte gather costs the CU's address path ~34 cycles per wave-load against 18 for any dword-aligned load of
//     up to 16 bytes (tools/src/probe_gather.hip), and 512 of them per CU and round is what the kernel waits for.  So a window is fetched
//     as the 12 ALIGNED bytes that contain it (the two pixels' 6 bytes start at byte 0..3 of them) and shifted into place with two
//     v_alignbit; the batch's last frame keeps the byte-aligned form (its shifted-back windows).
// Frame source: no trailing argument = DenseFrames (the kernel's name and code as before), crop_band_kernel<..., TableFrames> = the frame-
// table twin.  (Not a body function behind two kernels as crop_kernel / crop_fast_kernel: called through one, this kernel's register
// allocation moved -- 60 -> 64 VGPRs for crop_band_kernel<false, 6, 2, false> -- while as the kernel itself it compiles as before.)
template <class... Tab> struct FrameSource { using type = DenseFrames; };
template <class S> struct FrameSource<S> { using type = S; };
template <bool U8OUT, int LGT4, int IPT, bool ALIGNED, class... Tab>
__global__ __launch_bounds__(256) void crop_band_kernel(const unsigned char* __restrict__ frames, int H, int W,
                                                        const double* __restrict__ states, double factor,
                                                        float m0, float m1, float m2, float s0, float s1, float s2,
                                                        float* __restrict__ out, double* __restrict__ resize_factor) {
    using Src = typename FrameSource<Tab...>::type;
    constexpr int T4 = 1 << LGT4, T = 4 * T4, RPG = 256 >> LGT4, NROWS = IPT * RPG;      // rows per group of 256 items, rows per band
    static_assert(T <= 256 && (T * T4) % (IPT * 256) == 0, "a band is whole rows and the frame whole bands");
    const int b = blockIdx.y, tid = threadIdx.x;
    const FrameView fs = Src::shape(frames, H, W, b, gridDim.y);      // size and validity now, addresses below
    // VT_CROPF_DBG & 16 (timing build, uint8 form): s_memtime at the phase boundaries of every workgroup, written over the first 48 bytes of its band
    unsigned long long stamp_[7] = {0, 0, 0, 0, 0, 0, 0};
    auto stamp = [&](int i) {
        if constexpr ((VT_CROPF_DBG & 16) != 0) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamp_[i])::"memory");
    };
    stamp(0);
    __shared__ float norm_lut[U8OUT ? 1 : 3 * 256];
    __shared__ __attribute__((aligned(16))) unsigned xtab[T * 4];          // per output column: window byte offset, packed weights, right column's shift, -
    __shared__ __attribute__((aligned(16))) unsigned ytab[NROWS * 4];      // per output row of the band: byte offsets of its two source rows, their weights << 12
    unsigned char* const out8 = reinterpret_cast<unsigned char*>(out) + (size_t)b * T * T * 3;
    // not fill_norm_lut: through it crop_band_kernel<false, 6, 2, false> takes 64 VGPRs for 60 (tests/test_resource_usage.py holds it to the committed table)
    if constexpr (!U8OUT) {
        const float meanv[3] = {m0, m1, m2}, stdq[3] = {s0, s1, s2};
#pragma unroll
        for (int c = 0; c < 3; ++c) {       // Preprocessor.process on the 256 possible values: see fill_norm_lut
            float scaled = (float)tid * (1.0f / 255.0f);
            asm volatile("" : "+v"(scaled));
            float centred = scaled - meanv[c];
            asm volatile("" : "+v"(centred));
            norm_lut[c * 256 + tid] = centred / stdq[c];
        }
    }
    const int crop_sz = crop_side(states, b, factor);
    const int row0 = blockIdx.x * NROWS;                 // first output row of this band
    const int cg = tid & (T4 - 1), rl = tid >> LGT4;     // this thread's column group and its row inside a group of 256 items
    if (!(crop_sz >= 1) || !fs.ok) {        // see poison_item
        poison_band<U8OUT, T, IPT, RPG>(out, out8, resize_factor, b, row0, rl, cg);
        return;
    }
    const CropWindow g = crop_window(states, b, crop_sz, T, fs.H, fs.W);
    if (blockIdx.x == 0 && tid == 0) resize_factor[b] = (double)T / (double)crop_sz;
    if ((VT_CROPF_DBG & 16) != 0) { asm volatile("" ::"v"(g.x1), "v"(g.y1), "v"(g.scale)); stamp(1); }
    fill_band_tables<T, NROWS>(xtab, ytab, nullptr, row0, g, fs.pitch, 0u, 0u, frame_column_entry);
    __syncthreads();
    stamp(2);
    const FrameView fv = Src::view(frames, H, W, b, gridDim.y);
    const unsigned nrec = fv.nrec;
    const unsigned char* const fb = fv.base;
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(fb), 0, (int)nrec, 0x00020000);
    // ALIGNED: the same bytes through a descriptor whose base is the frame's address rounded DOWN to a dword; offsets carry the remainder
    const unsigned mis = (unsigned)(reinterpret_cast<unsigned long long>(fb) & 3ull);
    const auto rsrc_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(fb - mis), 0, (int)(nrec > 0xfffffff0u - 4u ? nrec : nrec + mis), 0x00020000);
    unsigned xo[4], wp[4], sh[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const u4v e = *reinterpret_cast<const u4v*>(xtab + 4 * (4 * cg + k));
        xo[k] = e.x + (ALIGNED ? mis : 0u); wp[k] = e.y; sh[k] = e.z;
    }
    // a window can cross the end of the buffer only in the batch's last frame (its last rows): there every load takes the byte-aligned,
    // shifted-back form.  The two forms are two instantiations of one body (AL: aligned 12-byte loads), so neither holds the other's registers.
    // ... and there only in a band that reads the frame's last source row (its windows end at most 11 + 3 bytes past their first byte: inside
    // the next row): every other band of the last frame takes the aligned form too -- the shifted form waits for each pair of windows before it
    // requests the next (the shift is part of the request), a chain of 4 IPT memory round trips that the whole launch waited for
    // FRAME TABLE: every frame's end may be the end of its allocation, so every frame takes this guard, on its own H, W and pitch.  Why the
    // aligned form reads inside [data, data + pitch (H - 1) + 3 W) when the guard lets it run (data 4-byte aligned: mis = 0): a window's
    // first byte is at o = row offset + 3 xb <= pitch ymax + 3 (W - 1) with ymax <= H - 2; its 12-byte aligned load starts at o & ~3 >= 0
    // and ends before o + 12 <= pitch (H - 2) + 3 W + 9 <= pitch (H - 1) + 3 W, as pitch >= 3 W >= 16 > 9.  Rows outside the valid range
    // read row 0.  And whatever the arithmetic, the buffer descriptor's bound (nrec = that extent) keeps every load inside the frame.
    bool last = fv.tail;      // dense: b == gridDim.y - 1
    if (ALIGNED && last) {
        if (band_last_source_row<NROWS>(row0, g) <= fs.H - 2 && fs.W * 3 >= 16) last = false;
    }
    unsigned two = 2u;
    asm volatile("" : "+v"(two));      // put_byte_shr2's shift operand has to live in a vector register
    const bool col_live = (wp[0] | wp[1] | wp[2] | wp[3]) != 0u;
    auto body = [&](auto al_c) {
        constexpr bool AL = decltype(al_c)::value;
        u2v q0[AL ? 1 : IPT][4], q1[AL ? 1 : IPT][4];
        u3v ra0[AL ? IPT : 1][4], ra1[AL ? IPT : 1][4];      // AL: the 12 aligned bytes around each window ...
        unsigned ro0[IPT], ro1[IPT];                          // ... and the item's row offsets: a window's shift is 8 x its offset's low two bits
        unsigned byw0[IPT], byw1[IPT];
        auto issue = [&](int j) {
            const u4v e = *reinterpret_cast<const u4v*>(ytab + 4 * (j * RPG + rl));
            byw0[j] = e.z; byw1[j] = e.w; ro0[j] = e.x; ro1[j] = e.y;
            // an item whose two rows or whose four columns all lie in the crop's zero padding (a window reaching over the frame's
            // border) weighs nothing: its loads are skipped, the products below are 0 x 0
            const bool live = ((e.z | e.w) != 0u) && col_live;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                unsigned o0 = e.x + xo[k], o1 = e.y + xo[k];
                if (!live) {
                    if constexpr (AL) { ra0[j][k] = u3v{0u, 0u, 0u}; ra1[j][k] = u3v{0u, 0u, 0u}; }
                    else { q0[j][k] = u2v{0u, 0u}; q1[j][k] = u2v{0u, 0u}; }
                } else
                if constexpr (AL) {
                    // raw 12 aligned bytes now; the funnel shift where they are used
                    ra0[j][k] = __builtin_amdgcn_raw_buffer_load_b96(rsrc_a, (int)(o0 & ~3u), 0, 0);
                    ra1[j][k] = __builtin_amdgcn_raw_buffer_load_b96(rsrc_a, (int)(o1 & ~3u), 0, 0);
                } else {
                    if (ALIGNED) { o0 -= mis; o1 -= mis; }
                    if (last) {
                        const unsigned ov0 = o0 + 8u > nrec ? o0 + 8u - nrec : 0u, ov1 = o1 + 8u > nrec ? o1 + 8u - nrec : 0u;
                        const u2v a = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)(o0 - ov0), 0, 0);
                        const u2v c = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)(o1 - ov1), 0, 0);
                        const unsigned long long wa = (((unsigned long long)a.y << 32) | a.x) >> (8u * ov0), wc = (((unsigned long long)c.y << 32) | c.x) >> (8u * ov1);
                        q0[j][k] = u2v{(unsigned)wa, (unsigned)(wa >> 32)};
                        q1[j][k] = u2v{(unsigned)wc, (unsigned)(wc >> 32)};
                    } else {
                        q0[j][k] = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)o0, 0, 0);
                        q1[j][k] = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)o1, 0, 0);
                    }
                }
            }
        };
        auto math = [&](int j) {
            const int oy = row0 + j * RPG + rl;
            float res[3][4];
            unsigned pk[3] = {0u, 0u, 0u};      // U8OUT: the 12 bytes of the item's four pixels, HWC
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                u2v w0, w1;
                if constexpr (AL) {      // v_alignbit reads bits [4:0] of its shift: 8 x (offset & 3)
                    const unsigned b0 = (ro0[j] + xo[k]) << 3, b1 = (ro1[j] + xo[k]) << 3;
                    w0 = u2v{__builtin_amdgcn_alignbit(ra0[j][k].y, ra0[j][k].x, b0), __builtin_amdgcn_alignbit(ra0[j][k].z, ra0[j][k].y, b0)};
                    w1 = u2v{__builtin_amdgcn_alignbit(ra1[j][k].y, ra1[j][k].x, b1), __builtin_amdgcn_alignbit(ra1[j][k].z, ra1[j][k].y, b1)};
                } else {
                    w0 = q0[j][k]; w1 = q1[j][k];
                }
                const unsigned l0 = w0.x, l1 = w1.x;
                const unsigned r0w = __builtin_amdgcn_alignbit(w0.y, l0, sh[k]);       // the window >> 0 or 24 bits
                const unsigned r1w = __builtin_amdgcn_alignbit(w1.y, l1, sh[k]);
                // item 7: not merged, see NOTES.md (crop kernels); as a helper it cost the fp32 forms with four items 92 VGPRs for 89
                const us2 wv = __builtin_bit_cast(us2, wp[k]);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const unsigned sel = 0x0c040c00u + 0x00010001u * (unsigned)c;       // [left pixel's channel c, 0, right pixel's channel c, 0]
                    const unsigned r0 = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, __builtin_amdgcn_perm(r0w, l0, sel)), wv, 0u, false);
                    const unsigned r1 = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, __builtin_amdgcn_perm(r1w, l1, sel)), wv, 0u, false);
                    const unsigned t0 = mulhi24(byw0[j], r0 & ~15u), t1 = mulhi24(byw1[j], r1 & ~15u);      // (b (r >> 4)) >> 16, see crop_fast_kernel
                    // t0 + t1 <= (by0 + by1) * 32640 >> 16 = 1020 (the weights of a pair sum to 2048, r >> 4 <= 255 * 128): the reference's
                    // saturation can never act, so no clamp here (crop_kernel / crop_fast_kernel keep theirs: same results)
                    if constexpr (U8OUT) {
                        put_byte_shr2(pk[(3 * k + c) >> 2], t0 + t1 + 2u, two, (3 * k + c) & 3);
                    } else {
                        const unsigned v4 = (t0 + t1 + 2u) & ~3u;
                        res[c][k] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(norm_lut) + c * 1024 + v4);
                    }
                }
            }
            if constexpr (U8OUT) {
                *reinterpret_cast<u3a*>(out8 + ((size_t)oy * T + 4 * cg) * 3) = u3a{pk[0], pk[1], pk[2]};
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) st4(out + (((size_t)b * 3 + c) * T + oy) * T + 4 * cg, f4{res[c][0], res[c][1], res[c][2], res[c][3]});
            }
        };
        // item 8: not merged, see NOTES.md (crop kernels); as a helper it cost the fp32 aligned forms with four items 92 VGPRs for 89
        // two items at a time (the conditional loads are waited for as a whole anyway): half the window registers, so that the kernel
        // stays within 128 registers = four workgroups per CU = ONE round of the 1024 bands of 256 G128 frames
        constexpr int HS = IPT < 2 ? IPT : 2;
#pragma unroll
        for (int h = 0; h < IPT; h += HS) {
#pragma unroll
            for (int j = 0; j < HS; ++j) issue(h + j);
            if ((VT_CROPF_DBG & 16) != 0 && h == 0) {
                stamp(3);                                   // the first half's loads issued
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                stamp(4);                                   // ... and here
            }
#pragma unroll
            for (int j = 0; j < HS; ++j) math(h + j);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    if (ALIGNED && !last) body(std::integral_constant<bool, ALIGNED>{});
    else body(std::false_type{});
    if constexpr ((VT_CROPF_DBG & 16) != 0 && U8OUT) {
        stamp(5);
        {   // where this workgroup ran: HW_ID (wave / SIMD / CU / SH / SE ids) and XCC_ID
            unsigned hw, xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)\n\ts_getreg_b32 %1, hwreg(HW_REG_XCC_ID)" : "=s"(hw), "=s"(xcc));
            stamp_[6] = ((unsigned long long)xcc << 32) | hw;
        }
        __syncthreads();
        if (tid == 0)
            for (int i = 0; i < 7; ++i) reinterpret_cast<unsigned long long*>(out8 + (size_t)row0 * T * 3)[i] = stamp_[i];
    }
}

// ---- pixel formats (vt_crop_images & co.): a (B,) vt_image table, one descriptor per sequence (include/vittrack.h).  Each descriptor
// denotes an RGB image rgb(d); the kernels below crop it with exactly the arithmetic of the kernels above -- only the fetch of a tap
// pixel differs: it is converted to an RGB dword (R | G << 8 | B << 16) first.  New kernels, not new frame sources of the bodies above:
// those bodies fetch a 3-byte pixel pair as one window, and the existing instantiations stay as they compile today.
// The planar 16-bit layouts: 32 | sub << 2 | dep, codes 32-46 with dep != 3 (include/vittrack.h)
__device__ __forceinline__ bool is_wide16(int fmt) { return fmt >= VT_PIX_I010 && fmt <= VT_PIX_GRAY16 && (fmt & 3) != 3; }
// ... and of those the LSB-aligned 10- and 12-bit ones, whose 8-bit sample is min(word >> (depth - 8), 255): the shift, 2 or 4; 0 for
// every layout whose samples are single bytes (the 16-bit ones of dep 2 included: the high byte)
__device__ __forceinline__ unsigned wide_shift(int fmt) { return is_wide16(fmt) && (fmt & 3) != 2 ? 2u + 2u * (unsigned)(fmt & 3) : 0u; }

struct ImageView {
    const unsigned char* p0;       // plane 0: the packed pixels, or the luma plane
    const unsigned char* p1;       // plane 1: NV12 / NV21 / P010 chroma pairs, or the first chroma plane of I420 / YV12 / I444 / I422, or the G plane
    unsigned pitch0, pitch1;       // bytes between rows
    unsigned nrec0, nrec1;         // each plane's extent, the bound of its buffer descriptor (loads beyond it return zero, fetch nothing)
    unsigned p2;                   // I420 / YV12: byte offset of the second chroma plane from p1 (pitch1 H / 2); inside nrec1.  The planar
                                   // layouts (RGBP / BGRP, I444 / I422): of the third plane (pitch1 H)
    int H, W, fmt, col;            // fmt: the layout (bits 0-7 of vt_image.format); col: matrix | range << 1 (0 = BT.601 limited)
    bool ok;                       // false: an unusable descriptor, poisoned like a too-small box
};
__device__ __forceinline__ ImageView image_view(const vt_image* images, int b) {
    // one descriptor per workgroup at a workgroup-uniform address: scalar loads
    const vt_image* const d = images + b;
    const unsigned char* const p0 = d->plane0;
    const unsigned char* const p1 = d->plane1;
    const int H = d->H, W = d->W;
    const unsigned word = (unsigned)d->format;
    const int fmt = (int)(word & 0xffu), mat = (int)((word >> 8) & 0xfu), rng = (int)((word >> 12) & 0xfu);
    const bool nv = fmt == VT_PIX_NV12 || fmt == VT_PIX_NV21, p010 = fmt == VT_PIX_P010;
    const bool pl = fmt == VT_PIX_I420 || fmt == VT_PIX_YV12, pk2 = fmt == VT_PIX_YUYV || fmt == VT_PIX_UYVY;
    // the planar layouts: three full-height planes of single bytes (I422: chroma planes of W / 2 bytes a row), read as single bytes,
    // hence no alignment rule (plane 1 of a contiguous (3, H, W) tensor of odd H W is at an odd address)
    const bool prgb = fmt == VT_PIX_RGBP || fmt == VT_PIX_BGRP, p422 = fmt == VT_PIX_I422, pln = prgb || fmt == VT_PIX_I444 || p422;
    // the wide family (codes 21-26, 32-46).  v3: three planes of single bytes, V first; sp: two planes, plane 1 of (U, V) pairs at full
    // height, in bytes (NV16 / NV24) or 16-bit words (P210 / P410); w16: planar 16-bit words, 32 | sub << 2 | dep (is_wide16), sub 0 /
    // 1 / 2 / 3 = 4:2:0 / 4:2:2 / 4:4:4 / luma only, dep 0 / 1 / 2 = 10 / 12 / 16 bits (3: unassigned).  c422 / c444: the chroma
    // columns of every wide layout.  lsb: the 10- and 12-bit words are fetched as aligned 16-bit loads -- even addresses, even pitches;
    // every other wide layout is read as single bytes at any address
    const bool v3 = fmt == VT_PIX_YV16 || fmt == VT_PIX_YV24, sp = fmt >= VT_PIX_NV16 && fmt <= VT_PIX_P410, sp16 = fmt >= VT_PIX_P210 && sp;
    const bool w16 = is_wide16(fmt);
    const int wsub = w16 ? (fmt >> 2) & 3 : -1;
    const bool lsb = wide_shift(fmt) != 0u;
    const bool c422 = fmt == VT_PIX_YV16 || fmt == VT_PIX_NV16 || fmt == VT_PIX_P210 || wsub == 1;
    const bool c444 = fmt == VT_PIX_YV24 || fmt == VT_PIX_NV24 || fmt == VT_PIX_P410 || wsub == 2;
    const bool wide = v3 || sp || w16;
    const bool sub420 = nv || p010 || pl || wsub == 0, yuv = sub420 || pk2 || (pln && !prgb) || (wide && wsub != 3);
    const long long bpp = (fmt == VT_PIX_RGBA || fmt == VT_PIX_BGRA) ? 4 : ((p010 || pk2 || sp16 || w16) ? 2 : ((nv || pl || pln || wide || fmt == VT_PIX_GRAY8) ? 1 : 3));
    const unsigned long long amask = (pln || wide) ? (lsb ? 1ull : 0ull) : 3ull;
    bool ok = ((fmt >= VT_PIX_RGB && fmt <= VT_PIX_NV21) || (fmt >= VT_PIX_I420 && fmt <= VT_PIX_GRAY8) || pln || wide) && (word >> 16) == 0u && mat <= 1 &&
              rng <= 1 && (yuv || (mat | rng) == 0) && d->reserved == 0 && H >= 1 && W >= 1 && H <= 0x10000000 && W <= 0x10000000 &&
              (!sub420 || ((H | W) & 1) == 0) && (!(pk2 || p422 || c422) || (W & 1) == 0);
    const long long row0 = bpp * W, pitch0 = d->pitch0 == 0 ? row0 : d->pitch0;
    ok = ok && pitch0 >= row0 && pitch0 <= 0xfffffff0ll && p0 != nullptr && (reinterpret_cast<unsigned long long>(p0) & amask) == 0 && !(lsb && (pitch0 & 1));
    const unsigned long long ext0 = ok ? (unsigned long long)pitch0 * (unsigned long long)(H - 1) + (unsigned long long)row0 : 0ull;
    ok = ok && ext0 <= 0xfffffff0ull;
    long long pitch1 = 0;
    unsigned long long ext1 = 0, p2 = 0;
    if (sub420 || pln || (wide && wsub != 3)) {
        // chroma: H / 2 rows of W bytes (NV12 / NV21) or 2 W bytes (P010); I420 / YV12: two planes of H / 2 rows of W / 2 bytes back
        // to back at one pitch, i.e. H rows, and the extent covers both; the planar layouts: two planes of H rows back to back, 2 H rows.
        // The wide family: W / 2 (4:2:0, 4:2:2) or W (4:4:4) chroma samples a row per plane, twice that in a plane of pairs, bytes
        // doubled in 16-bit words; three-plane layouts as I420 (4:2:0) or the planar layouts, planes of pairs H rows
        const long long cw = (c444 ? (long long)W : W / 2) * (sp ? 2ll : 1ll) * ((sp16 || w16) ? 2ll : 1ll);
        const long long row1 = wide ? cw : (p010 ? 2ll * W : ((pl || p422) ? W / 2 : (long long)W));
        const bool three = pl || pln || v3 || w16;      // a trailing chroma plane: pitch1 x chroma rows behind plane 1
        const long long crows = sub420 ? H / 2 : H;
        const long long rows1 = three ? 2 * crows : crows;
        pitch1 = d->pitch1 == 0 ? row1 : d->pitch1;
        ok = ok && pitch1 >= row1 && pitch1 <= 0xfffffff0ll && p1 != nullptr && (reinterpret_cast<unsigned long long>(p1) & amask) == 0 && !(lsb && (pitch1 & 1));
        ext1 = ok ? (unsigned long long)pitch1 * (unsigned long long)(rows1 - 1) + (unsigned long long)row1 : 0ull;
        ok = ok && ext1 <= 0xfffffff0ull;
        p2 = (ok && three) ? (unsigned long long)pitch1 * (unsigned long long)crows : 0ull;
    }
    return ImageView{p0, p1, ok ? (unsigned)pitch0 : 0u, ok ? (unsigned)pitch1 : 0u, ok ? (unsigned)ext0 : 0u, ok ? (unsigned)ext1 : 0u,
                     (unsigned)p2, ok ? H : 1, ok ? W : 1, fmt, ok ? (mat | (rng << 1)) : 0, ok};
}
// The six first layouts (RGB ... NV21, no colour bits) as crop_band_image_kernel has always read them: its own view, so that its code
// does not change with the layouts added to image_view
struct ImageView6 {
    const unsigned char* p0;       // plane 0: the packed pixels, or NV12 / NV21 luma
    const unsigned char* p1;       // plane 1: NV12 / NV21 chroma pairs
    unsigned pitch0, pitch1;       // bytes between rows
    unsigned nrec0, nrec1;         // each plane's extent, the bound of its buffer descriptor (loads beyond it return zero, fetch nothing)
    int H, W, fmt;
    bool ok;                       // false: an unusable descriptor, poisoned like a too-small box
};
__device__ __forceinline__ ImageView6 image_view6(const vt_image* images, int b) {
    // one descriptor per workgroup at a workgroup-uniform address: scalar loads
    const vt_image* const d = images + b;
    const unsigned char* const p0 = d->plane0;
    const unsigned char* const p1 = d->plane1;
    const int H = d->H, W = d->W, fmt = d->format;
    const bool nv = fmt == VT_PIX_NV12 || fmt == VT_PIX_NV21;
    const long long bpp = (fmt == VT_PIX_RGBA || fmt == VT_PIX_BGRA) ? 4 : (nv ? 1 : 3);
    bool ok = fmt >= VT_PIX_RGB && fmt <= VT_PIX_NV21 && d->reserved == 0 && H >= 1 && W >= 1 && H <= 0x10000000 && W <= 0x10000000 &&
              (!nv || ((H | W) & 1) == 0);
    const long long row0 = bpp * W, pitch0 = d->pitch0 == 0 ? row0 : d->pitch0;
    ok = ok && pitch0 >= row0 && pitch0 <= 0xfffffff0ll && p0 != nullptr && (reinterpret_cast<unsigned long long>(p0) & 3ull) == 0;
    const unsigned long long ext0 = ok ? (unsigned long long)pitch0 * (unsigned long long)(H - 1) + (unsigned long long)row0 : 0ull;
    ok = ok && ext0 <= 0xfffffff0ull;
    long long pitch1 = 0;
    unsigned long long ext1 = 0;
    if (nv) {      // chroma: H / 2 rows of W bytes
        pitch1 = d->pitch1 == 0 ? (long long)W : d->pitch1;
        ok = ok && pitch1 >= W && pitch1 <= 0xfffffff0ll && p1 != nullptr && (reinterpret_cast<unsigned long long>(p1) & 3ull) == 0;
        ext1 = ok ? (unsigned long long)pitch1 * (unsigned long long)(H / 2 - 1) + (unsigned long long)W : 0ull;
        ok = ok && ext1 <= 0xfffffff0ull;
    }
    return ImageView6{p0, p1, ok ? (unsigned)pitch0 : 0u, ok ? (unsigned)pitch1 : 0u, ok ? (unsigned)ext0 : 0u, ok ? (unsigned)ext1 : 0u,
                     ok ? H : 1, ok ? W : 1, fmt, ok};
}
// BT.601 limited range in OpenCV's fixed point (include/vittrack.h): the literals of crop_band_image_kernel's NV12 / NV21 family.  (Every
// other path -- crop_image_kernel, crop_band_image_ext -- takes the coefficient row of its descriptor from yuv_coef below, whose BT.601
// limited row is these numbers.)  The chroma terms of a pair, rounding constant included ...
struct ChromaTerms { int r, g, b; };
__device__ __forceinline__ ChromaTerms chroma_terms(unsigned u8, unsigned v8) {
    const int u = (int)u8 - 128, v = (int)v8 - 128;
    return ChromaTerms{1673527 * v + (1 << 19), -852492 * v - 409993 * u + (1 << 19), 2116026 * u + (1 << 19)};
}
// ... and one pixel: R | G << 8 | B << 16
__device__ __forceinline__ unsigned yuv_rgb(unsigned y8, const ChromaTerms& c) {
    const int yy = (int)(y8 > 16u ? y8 - 16u : 0u) * 1220542;
    auto ch = [](int s) { s >>= 20; return (unsigned)(s < 0 ? 0 : (s > 255 ? 255 : s)); };
    return ch(yy + c.r) | (ch(yy + c.g) << 8) | (ch(yy + c.b) << 16);
}
// The other colour rows (include/vittrack.h): round(x 2^20) of the exact rationals.  Uniform in a workgroup: scalar selects, SGPRs.
struct YuvCoef { int cy, cvr, cvg, cug, cub; unsigned yoff; };
__device__ __forceinline__ YuvCoef yuv_coef(int col) {      // col: matrix | range << 1
    const bool m709 = (col & 1) != 0, full = (col & 2) != 0;
    return YuvCoef{full ? 1048576 : (m709 ? 1220945 : 1220542),
                   m709 ? (full ? 1651297 : 1879825) : (full ? 1470104 : 1673527),
                   m709 ? (full ? 490864 : 558796) : (full ? 748826 : 852492),
                   m709 ? (full ? 196424 : 223607) : (full ? 360853 : 409993),
                   m709 ? (full ? 1945738 : 2215014) : (full ? 1858077 : 2116026),
                   full ? 0u : 16u};
}
__device__ __forceinline__ ChromaTerms chroma_terms(unsigned u8, unsigned v8, const YuvCoef& k) {
    const int u = (int)u8 - 128, v = (int)v8 - 128;
    return ChromaTerms{k.cvr * v + (1 << 19), -k.cvg * v - k.cug * u + (1 << 19), k.cub * u + (1 << 19)};
}
__device__ __forceinline__ unsigned yuv_rgb(unsigned y8, const ChromaTerms& c, const YuvCoef& k) {
    const int yy = (int)(y8 > k.yoff ? y8 - k.yoff : 0u) * k.cy;
    auto ch = [](int s) { s >>= 20; return (unsigned)(s < 0 ? 0 : (s > 255 ? 255 : s)); };
    return ch(yy + c.r) | (ch(yy + c.g) << 8) | (ch(yy + c.b) << 16);
}
// Where the three samples of pixel (x, y) of a YUV layout lie, as uniform multipliers: luma at byte y pitch0 + x ymul + yadd of plane 0;
// U and V at bytes (y >> cys) cpitch + (x >> cxs) cmul + uoff / voff of plane 1 (or, c0: of plane 0 -- the packed 4:2:2 layouts).
// P010: the sample is the high byte of each little-endian 16-bit word, hence the odd offsets.
// I444: every pixel its own chroma (cxs = 0), the V plane pitch1 H bytes behind the U plane.  Planar RGB is addressed exactly so -- plane
// 0 where I444 keeps luma, the two trailing planes where it keeps U and V -- and differs in what the three bytes mean (is_planar_rgb).
// The wide family.  YV16 / YV24: I422 / I444 with U and V exchanged.  NV16 / NV24: NV12's pairs at full height (cys = 0), NV24 a pair
// a pixel.  P210 / P410: those in 16-bit words, the high byte of each as P010.  Planar 16-bit (is_wide16): I420 / I422 / I444 / GRAY8
// in 16-bit words -- dep 2: the high bytes (odd offsets), fetched as bytes; dep 0 / 1: the offsets are those of the aligned words
// themselves, fetched by the 16-bit family of the two image kernels (wide_shift).
struct YuvLayout { unsigned ymul, yadd, cys, cpitch, cmul, uoff, voff, cxs; bool c0; };
__device__ __forceinline__ YuvLayout yuv_layout(const ImageView& iv) {
    if (is_wide16(iv.fmt)) {
        const unsigned sub = ((unsigned)iv.fmt >> 2) & 3u, hb = ((unsigned)iv.fmt & 3u) == 2u ? 1u : 0u;
        if (sub == 3u) return YuvLayout{2u, hb, 0u, 0u, 0u, 0u, 0u, 1u, true};      // luma only
        return YuvLayout{2u, hb, sub == 0u ? 1u : 0u, iv.pitch1, 2u, hb, iv.p2 + hb, sub == 2u ? 0u : 1u, false};
    }
    switch (iv.fmt) {
        case VT_PIX_YV16: return YuvLayout{1u, 0u, 0u, iv.pitch1, 1u, iv.p2, 0u, 1u, false};
        case VT_PIX_YV24: return YuvLayout{1u, 0u, 0u, iv.pitch1, 1u, iv.p2, 0u, 0u, false};
        case VT_PIX_NV16: return YuvLayout{1u, 0u, 0u, iv.pitch1, 2u, 0u, 1u, 1u, false};
        case VT_PIX_NV24: return YuvLayout{1u, 0u, 0u, iv.pitch1, 2u, 0u, 1u, 0u, false};
        case VT_PIX_P210: return YuvLayout{2u, 1u, 0u, iv.pitch1, 4u, 1u, 3u, 1u, false};
        case VT_PIX_P410: return YuvLayout{2u, 1u, 0u, iv.pitch1, 4u, 1u, 3u, 0u, false};
        case VT_PIX_NV21: return YuvLayout{1u, 0u, 1u, iv.pitch1, 2u, 1u, 0u, 1u, false};
        case VT_PIX_I420: return YuvLayout{1u, 0u, 1u, iv.pitch1, 1u, 0u, iv.p2, 1u, false};
        case VT_PIX_YV12: return YuvLayout{1u, 0u, 1u, iv.pitch1, 1u, iv.p2, 0u, 1u, false};
        case VT_PIX_YUYV: return YuvLayout{2u, 0u, 0u, iv.pitch0, 4u, 1u, 3u, 1u, true};
        case VT_PIX_UYVY: return YuvLayout{2u, 1u, 0u, iv.pitch0, 4u, 0u, 2u, 1u, true};
        case VT_PIX_P010: return YuvLayout{2u, 1u, 1u, iv.pitch1, 4u, 1u, 3u, 1u, false};
        case VT_PIX_GRAY8: return YuvLayout{1u, 0u, 0u, 0u, 0u, 0u, 0u, 1u, true};      // luma only
        case VT_PIX_I422: return YuvLayout{1u, 0u, 0u, iv.pitch1, 1u, 0u, iv.p2, 1u, false};
        case VT_PIX_RGBP:
        case VT_PIX_BGRP:
        case VT_PIX_I444: return YuvLayout{1u, 0u, 0u, iv.pitch1, 1u, 0u, iv.p2, 0u, false};
        default: return YuvLayout{1u, 0u, 1u, iv.pitch1, 2u, 0u, 1u, 1u, false};         // NV12
    }
}
// Planar RGB (RGBP / BGRP): the bytes at yuv_layout's luma / U / V places are the channels themselves -- plane 0, G, the third plane
__device__ __forceinline__ bool is_planar_rgb(int fmt) { return fmt == VT_PIX_RGBP || fmt == VT_PIX_BGRP; }
__device__ __forceinline__ unsigned planar_rgb(unsigned a, unsigned g, unsigned c, bool bgr) {      // R | G << 8 | B << 16
    return bgr ? (c | (g << 8) | (a << 16)) : (a | (g << 8) | (c << 16));
}
__device__ __forceinline__ bool is_yuv_layout(int fmt) {
    return fmt == VT_PIX_NV12 || fmt == VT_PIX_NV21 || (fmt >= VT_PIX_I420 && fmt <= VT_PIX_P010) || fmt == VT_PIX_I444 || fmt == VT_PIX_I422 ||
           (fmt >= VT_PIX_YV16 && fmt <= VT_PIX_P410) || (fmt >= VT_PIX_I010 && fmt < VT_PIX_GRAY10);
}
// luma only: rgb = (Y, Y, Y), Y the 8-bit sample at yuv_layout's luma place
__device__ __forceinline__ bool is_gray_layout(int fmt) { return fmt == VT_PIX_GRAY8 || fmt >= VT_PIX_GRAY10; }
// The tracker's tail clips against each sequence's own frame size (TrackTail::frames): the crop of vt_track_step_images writes the
// sizes of its descriptors into a vt_frame-shaped table as it reads them (sizes may be null: vt_crop_images)
__device__ __forceinline__ void image_sizes_out(vt_frame* sizes, const vt_image* images, int b) {
    if (sizes != nullptr) sizes[b] = vt_frame{nullptr, images[b].H, images[b].W, 0};
}

// crop_image_kernel: crop_kernel on a vt_image table -- any T, fp32 crop or (U8OUT) uint8 patch; vt_crop_images at the sizes the band
// kernel does not take, and the template crop of BatchedVitTracker.initialize.  One thread = four consecutive output pixels of a row,
// as crop_kernel; every tap pixel is fetched as single bytes (buffer bounds: a byte beyond its plane reads as zero and is not fetched)
// and converted to RGB, then crop_kernel's arithmetic, clamp included.
template <bool U8OUT = false>
__global__ __launch_bounds__(256) void crop_image_kernel(const vt_image* __restrict__ images, vt_frame* __restrict__ sizes,
                                                         const double* __restrict__ states, double factor, int T,
                                                         float m0, float m1, float m2, float s0, float s1, float s2,
                                                         float* __restrict__ out, double* __restrict__ resize_factor) {
    const int b = blockIdx.y;
    const ImageView iv = image_view(images, b);
    __shared__ float norm_lut[U8OUT ? 1 : 3 * 256];
    if constexpr (!U8OUT) {
        fill_norm_lut(norm_lut, m0, m1, m2, s0, s1, s2);
        __syncthreads();
    }
    unsigned char* const out8 = reinterpret_cast<unsigned char*>(out) + (size_t)b * T * T * 3;
    const int crop_sz = crop_side(states, b, factor);
    const int T4 = (T + 3) >> 2;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx == 0) image_sizes_out(sizes, images, b);
    if (!(crop_sz >= 1) || !iv.ok) {        // see poison_item
        if (idx == 0) resize_factor[b] = __builtin_nan("");
        if (idx < T * T4) poison_item<U8OUT, true>(out, out8, b, T, idx / T4, (idx - idx / T4 * T4) * 4);
        return;
    }
    const CropWindow g = crop_window(states, b, crop_sz, T, iv.H, iv.W);
    if (idx == 0) resize_factor[b] = (double)T / (double)crop_sz;
    if (idx >= T * T4) return;
    const int oy = idx / T4, ox0 = (idx - oy * T4) * 4;
    int sy0, sy1, by0, by1;
    lin_coeff(oy, g.crop_sz, g.scale, sy0, sy1, by0, by1);
    const auto rs0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(iv.p0), 0, (int)iv.nrec0, 0x00020000);
    auto byte0 = [&](unsigned o) { return (unsigned)__builtin_amdgcn_raw_buffer_load_b8(rs0, (int)o, 0, 0) & 0xffu; };
    const int fmt = iv.fmt;
    const bool swap = fmt == VT_PIX_BGR || fmt == VT_PIX_BGRA;
    const bool yuvf = is_yuv_layout(fmt), prgb = is_planar_rgb(fmt);
    const YuvLayout yl = yuv_layout(iv);
    const YuvCoef kc = yuv_coef(iv.col);
    const bool c1 = !yl.c0 && iv.p1 != nullptr;      // where the chroma samples are: plane 1, or plane 0 (packed 4:2:2)
    const auto rsc = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(c1 ? iv.p1 : iv.p0), 0, (int)(c1 ? iv.nrec1 : iv.nrec0), 0x00020000);
    // The 10- and 12-bit planar layouts: one 16-bit load a sample, s8 = min(word >> wsh, 255).  Bound: planes and pitches are even
    // (image_view), so a word's offset pitch y + 2 x is even and at most extent - 2, the extent pitch (rows - 1) + 2 (samples a row)
    // being even: no load starts at the extent's last byte, and none crosses it.
    const unsigned wsh = wide_shift(fmt);
    auto word0 = [&](unsigned o) { const unsigned w = ((unsigned)__builtin_amdgcn_raw_buffer_load_b16(rs0, (int)o, 0, 0) & 0xffffu) >> wsh; return w < 255u ? w : 255u; };
    auto wordc = [&](unsigned o) { const unsigned w = ((unsigned)__builtin_amdgcn_raw_buffer_load_b16(rsc, (int)o, 0, 0) & 0xffffu) >> wsh; return w < 255u ? w : 255u; };
    auto pixel = [&](int x, int y) -> unsigned {      // rgb(d) at (x, y), inside the image
        if (wsh != 0u) {         // uniform: the 16-bit fetch family
            const unsigned a = word0((unsigned)y * iv.pitch0 + (unsigned)x * 2u);
            if (!yuvf) return a * 0x010101u;      // GRAY10 / GRAY12
            const unsigned co = ((unsigned)y >> yl.cys) * yl.cpitch + ((unsigned)x >> yl.cxs) * 2u;
            return yuv_rgb(a, chroma_terms(wordc(co), wordc(co + yl.voff), kc), kc);
        }
        if (yuvf || prgb) {      // every sample a single byte: see yuv_layout
            const unsigned co = ((unsigned)y >> yl.cys) * yl.cpitch + ((unsigned)x >> yl.cxs) * yl.cmul;
            const unsigned u = (unsigned)__builtin_amdgcn_raw_buffer_load_b8(rsc, (int)(co + yl.uoff), 0, 0) & 0xffu;
            const unsigned v = (unsigned)__builtin_amdgcn_raw_buffer_load_b8(rsc, (int)(co + yl.voff), 0, 0) & 0xffu;
            const unsigned a = byte0((unsigned)y * iv.pitch0 + (unsigned)x * yl.ymul + yl.yadd);
            if (prgb) return planar_rgb(a, u, v, fmt == VT_PIX_BGRP);
            return yuv_rgb(a, chroma_terms(u, v, kc), kc);
        }
        if (fmt == VT_PIX_GRAY16) return byte0((unsigned)y * iv.pitch0 + (unsigned)x * 2u + 1u) * 0x010101u;      // the high byte
        if (fmt == VT_PIX_GRAY8) return byte0((unsigned)y * iv.pitch0 + (unsigned)x) * 0x010101u;
        const unsigned o = (unsigned)y * iv.pitch0 + (unsigned)x * ((fmt == VT_PIX_RGBA || fmt == VT_PIX_BGRA) ? 4u : 3u);
        const unsigned a = byte0(o), gr = byte0(o + 1u), c = byte0(o + 2u);
        return swap ? (c | (gr << 8) | (a << 16)) : (a | (gr << 8) | (c << 16));
    };
    const int yy0 = g.y1 + sy0, yy1 = g.y1 + sy1;
    const bool vr0 = yy0 >= g.vy0 && yy0 < g.vy1, vr1 = yy1 >= g.vy0 && yy1 < g.vy1;
    float res[3][4];
    unsigned pk[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ox = ox0 + k < T ? ox0 + k : T - 1;
        int sx0, sx1, ax0, ax1;
        lin_coeff(ox, g.crop_sz, g.scale, sx0, sx1, ax0, ax1);
        const int xx0 = g.x1 + sx0, xx1 = g.x1 + sx1;
        const bool vc0 = xx0 >= g.vx0 && xx0 < g.vx1, vc1 = xx1 >= g.vx0 && xx1 < g.vx1;
        // pixel (cy, cx) of the zero-padded crop: rgb(d) inside the valid range, 0 outside (all channels)
        const unsigned l0 = vr0 && vc0 ? pixel(xx0, yy0) : 0u, l1 = vr1 && vc0 ? pixel(xx0, yy1) : 0u;
        const unsigned r0w = vr0 && vc1 ? pixel(xx1, yy0) : 0u, r1w = vr1 && vc1 ? pixel(xx1, yy1) : 0u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {       // crop_kernel's arithmetic
            // item 7b: not merged, see NOTES.md (crop kernels)
            const int p00 = (int)((l0 >> (8 * c)) & 0xffu), p01 = (int)((r0w >> (8 * c)) & 0xffu);
            const int p10 = (int)((l1 >> (8 * c)) & 0xffu), p11 = (int)((r1w >> (8 * c)) & 0xffu);
            const int r0 = __mul24(p00, ax0) + __mul24(p01, ax1);
            const int r1 = __mul24(p10, ax0) + __mul24(p11, ax1);
            int v = ((__mul24(by0, r0 >> 4) >> 16) + (__mul24(by1, r1 >> 4) >> 16) + 2) >> 2;
            v = v < 0 ? 0 : (v > 255 ? 255 : v);
            if constexpr (U8OUT) pk[(3 * k + c) >> 2] |= (unsigned)v << (8 * ((3 * k + c) & 3));
            else res[c][k] = norm_lut[c * 256 + v];
        }
    }
    if constexpr (U8OUT) {
        unsigned char* o = out8 + ((size_t)oy * T + ox0) * 3;
        if ((T & 3) == 0) {
            *reinterpret_cast<u3a*>(o) = u3a{pk[0], pk[1], pk[2]};
        } else {
            for (int i = 0; i < 12 && ox0 + i / 3 < T; ++i) o[i] = (unsigned char)(pk[i >> 2] >> (8 * (i & 3)));
        }
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float* o = out + (((size_t)b * 3 + c) * T + oy) * T + ox0;
        if ((T & 3) == 0) {
            st4(o, f4{res[c][0], res[c][1], res[c][2], res[c][3]});
        } else {
            for (int k = 0; k < 4 && ox0 + k < T; ++k) o[k] = res[c][k];
        }
    }
}

// crop_band_image_ext: the band crop of every format word beyond the six first layouts -- NV12 / NV21 under BT.709 or full range, P010,
// I420 / YV12, YUYV / UYVY, GRAY8 -- called by crop_band_image_kernel (below) behind one uniform branch, with the same bands, tables,
// arithmetic and results.  A body of its own, so that the code of the six first layouts stays what it was.  Families, each behind a
// uniform branch (the format is uniform in a workgroup):
//   - NV12 / NV21, the three other colour rows: crop_band_image_kernel's aligned 8-byte luma and chroma windows and its GUARD rule; the
//     five coefficients and the luma floor come from SGPRs (yuv_coef) instead of literals
//   - P010: aligned windows of its own (8 bytes of luma, 12 of chroma), one item at a time; derivation at the lambda
//   - I420 / YV12, YUYV / UYVY, GRAY8, and the planar layouts (I444 / I422, RGBP / BGRP): every sample of a tap as a single byte at the
//     offsets yuv_layout gives, one item at a time
// LDS: the tables below are this body's own, next to the kernel's (a workgroup allocates both sets: 2 x 7.4 KB at most, T = 256 in the
// fp32 form; four workgroups a CU stay far inside the CU's LDS) -- the kernel's code was to stay as it compiles, its arrays included.
// (`four` and `swap` below are false for every word that reaches a family here: an RGB layout with colour bits is poisoned first.)
// xtab / ytab as in crop_band_kernel; ctab holds per output row the chroma-row offsets of its two source rows ((y >> cys) * cpitch of
// yuv_layout: plane 1 for the 4:2:0 layouts, plane 0 for packed 4:2:2).
template <bool U8OUT, int LGT4, int IPT>
__device__ __forceinline__ void crop_band_image_ext(const vt_image* __restrict__ images, vt_frame* __restrict__ sizes,
                                                              const double* __restrict__ states, double factor,
                                                              float m0, float m1, float m2, float s0, float s1, float s2,
                                                              float* __restrict__ out, double* __restrict__ resize_factor) {
    constexpr int T4 = 1 << LGT4, T = 4 * T4, RPG = 256 >> LGT4, NROWS = IPT * RPG;
    static_assert(T <= 256 && (T * T4) % (IPT * 256) == 0, "a band is whole rows and the frame whole bands");
    const int b = blockIdx.y, tid = threadIdx.x;
    const ImageView iv = image_view(images, b);
    // item 11: not merged, see NOTES.md (crop kernels)
    __shared__ float norm_lut[U8OUT ? 1 : 3 * 256];
    __shared__ __attribute__((aligned(16))) unsigned xtab[T * 4];          // per output column: plane-0 byte offset of the window, packed weights, steps, chroma offset
    __shared__ __attribute__((aligned(16))) unsigned ytab[NROWS * 4];      // per output row: plane-0 offsets of its two source rows, their weights << 12
    __shared__ __attribute__((aligned(8))) unsigned ctab[NROWS * 2];       // per output row: chroma-row offsets of its two source rows (NV12 / NV21)
    unsigned char* const out8 = reinterpret_cast<unsigned char*>(out) + (size_t)b * T * T * 3;
    if constexpr (!U8OUT) fill_norm_lut(norm_lut, m0, m1, m2, s0, s1, s2);
    const int crop_sz = crop_side(states, b, factor);
    const int row0 = blockIdx.x * NROWS;
    const int cg = tid & (T4 - 1), rl = tid >> LGT4;
    if (blockIdx.x == 0 && tid == 0) image_sizes_out(sizes, images, b);
    if (!(crop_sz >= 1) || !iv.ok) {        // see poison_item
        poison_band<U8OUT, T, IPT, RPG>(out, out8, resize_factor, b, row0, rl, cg);
        return;
    }
    const int fmt = iv.fmt;
    const bool nv = fmt == VT_PIX_NV12 || fmt == VT_PIX_NV21, four = fmt == VT_PIX_RGBA || fmt == VT_PIX_BGRA;
    const bool newf = fmt >= VT_PIX_I420;      // I420 / YV12, YUYV / UYVY, P010, GRAY8, the planar layouts: their column and row entries follow yuv_layout
    const YuvLayout yl = yuv_layout(iv);
    const YuvCoef kc = yuv_coef(iv.col);
    const unsigned bpp = (nv || newf) ? yl.ymul : (four ? 4u : 3u);
    const CropWindow g = crop_window(states, b, crop_sz, T, iv.H, iv.W);
    if (blockIdx.x == 0 && tid == 0) resize_factor[b] = (double)T / (double)crop_sz;
    fill_band_tables<T, NROWS>(xtab, ytab, ctab, row0, g, iv.pitch0, newf ? yl.cys : 1u, newf ? yl.cpitch : iv.pitch1,
                               [&](const ColumnTap& t) { return image_column_entry(t, bpp, newf ? yl.yadd : 0u, newf ? yl.cmul : 2u, newf ? yl.cxs : 1u); });
    __syncthreads();
    const auto rs0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(iv.p0), 0, (int)iv.nrec0, 0x00020000);
    const bool c1 = nv || (newf && !yl.c0);      // chroma in plane 1; else (packed 4:2:2) in plane 0
    const unsigned nrecc = c1 ? iv.nrec1 : (newf ? iv.nrec0 : 0u);
    const auto rs1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(c1 ? iv.p1 : iv.p0), 0, (int)nrecc, 0x00020000);
    unsigned xo[4], wp[4], st[4], xc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const u4v e = *reinterpret_cast<const u4v*>(xtab + 4 * (4 * cg + k));
        xo[k] = e.x; wp[k] = e.y; st[k] = e.z; xc[k] = e.w;
    }
    // the byte of each channel in an RGB-ordered (or, swapped, BGR-ordered) pixel dword: v_perm_b32 selectors
    // [left pixel's channel, 0, right pixel's channel, 0], uniform
    const bool swap = fmt == VT_PIX_BGR || fmt == VT_PIX_BGRA;
    unsigned sel[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) sel[c] = 0x0c040c00u + 0x00010001u * (unsigned)(swap ? 2 - c : c);
    const unsigned ush = fmt == VT_PIX_NV21 ? 8u : 0u;      // bit offset of U in a chroma pair (V at the other byte)
    unsigned two = 2u;
    asm volatile("" : "+v"(two));
    const bool col_live = (wp[0] | wp[1] | wp[2] | wp[3]) != 0u;
    // the output of one item from its four tap-pair dwords per row (l = left tap, r = right tap: R | G << 8 | B << 16)
    // item 7: not merged, see NOTES.md (crop kernels)
    auto finish = [&](int j, const unsigned (&l0)[4], const unsigned (&r0w)[4], const unsigned (&l1)[4], const unsigned (&r1w)[4],
                      unsigned byw0, unsigned byw1) {
        const int oy = row0 + j * RPG + rl;
        float res[3][4];
        unsigned pk[3] = {0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const us2 wv = __builtin_bit_cast(us2, wp[k]);
#pragma unroll
            for (int c = 0; c < 3; ++c) {       // crop_band_kernel's arithmetic
                const unsigned r0 = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, __builtin_amdgcn_perm(r0w[k], l0[k], sel[c])), wv, 0u, false);
                const unsigned r1 = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, __builtin_amdgcn_perm(r1w[k], l1[k], sel[c])), wv, 0u, false);
                const unsigned t0 = mulhi24(byw0, r0 & ~15u), t1 = mulhi24(byw1, r1 & ~15u);
                if constexpr (U8OUT) {
                    put_byte_shr2(pk[(3 * k + c) >> 2], t0 + t1 + 2u, two, (3 * k + c) & 3);
                } else {
                    const unsigned v4 = (t0 + t1 + 2u) & ~3u;
                    res[c][k] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(norm_lut) + c * 1024 + v4);
                }
            }
        }
        if constexpr (U8OUT) {
            *reinterpret_cast<u3a*>(out8 + ((size_t)oy * T + 4 * cg) * 3) = u3a{pk[0], pk[1], pk[2]};
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) st4(out + (((size_t)b * 3 + c) * T + oy) * T + 4 * cg, f4{res[c][0], res[c][1], res[c][2], res[c][3]});
        }
    };
    constexpr int HS = IPT < 2 ? IPT : 2;      // two items at a time, as crop_band_kernel
    // NV12 / NV21; GUARD: windows that would cross their plane's end are read as single bytes
    // VC: one of the three other colour rows -- the same windows, the coefficients and the luma floor from kc (SGPRs) instead of literals
    // items 9 and 8: not merged, see NOTES.md (crop kernels)
    auto yuv = [&](auto guard_c) {
        constexpr bool GUARD = decltype(guard_c)::value;
        u2v ya0[IPT][4], ya1[IPT][4], ca0[IPT][4], ca1[IPT][4];
        unsigned ro0[IPT], ro1[IPT], co0[IPT], co1[IPT], byw0[IPT], byw1[IPT];
        auto load8 = [&](const auto& rs, unsigned o, unsigned nrec) -> u2v {      // the 8 bytes from the dword that holds byte o
            const unsigned a = o & ~3u;
            if (!GUARD || a + 8u <= nrec) return __builtin_amdgcn_raw_buffer_load_b64(rs, (int)a, 0, 0);
            unsigned lo = 0u, hi = 0u;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                lo |= ((unsigned)__builtin_amdgcn_raw_buffer_load_b8(rs, (int)(a + i), 0, 0) & 0xffu) << (8 * i);
                hi |= ((unsigned)__builtin_amdgcn_raw_buffer_load_b8(rs, (int)(a + 4 + i), 0, 0) & 0xffu) << (8 * i);
            }
            return u2v{lo, hi};
        };
        auto issue = [&](int j) {
            const u4v e = *reinterpret_cast<const u4v*>(ytab + 4 * (j * RPG + rl));
            const u2v cr = *reinterpret_cast<const u2v*>(ctab + 2 * (j * RPG + rl));
            ro0[j] = e.x; ro1[j] = e.y; byw0[j] = e.z; byw1[j] = e.w; co0[j] = cr.x; co1[j] = cr.y;
            const bool live = ((e.z | e.w) != 0u) && col_live;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!live) {      // (one assignment each: chained, they kept the arrays in scratch)
                    ya0[j][k] = u2v{0u, 0u}; ya1[j][k] = u2v{0u, 0u}; ca0[j][k] = u2v{0u, 0u}; ca1[j][k] = u2v{0u, 0u};
                    continue;
                }
                ya0[j][k] = load8(rs0, e.x + xo[k], iv.nrec0);
                ya1[j][k] = load8(rs0, e.y + xo[k], iv.nrec0);
                ca0[j][k] = load8(rs1, cr.x + xc[k], iv.nrec1);
                ca1[j][k] = load8(rs1, cr.y + xc[k], iv.nrec1);
            }
        };
        auto taps = [&](const u2v& yw, const u2v& cw, unsigned yo, unsigned co, unsigned s, unsigned& l, unsigned& r) {
            const unsigned y = __builtin_amdgcn_alignbit(yw.y, yw.x, yo << 3);      // luma of the left tap at byte 0, the next pixel's at byte 1
            const unsigned c = __builtin_amdgcn_alignbit(cw.y, cw.x, co << 3);      // the left tap's chroma pair at bytes 0-1, the next pair at 2-3
            const unsigned cl = c & 0xffffu, cr = (s & 2u) ? c >> 16 : cl;
            l = yuv_rgb(y & 0xffu, chroma_terms((cl >> ush) & 0xffu, (cl >> (8u - ush)) & 0xffu, kc), kc);
            r = yuv_rgb((s & 1u) ? (y >> 8) & 0xffu : y & 0xffu, chroma_terms((cr >> ush) & 0xffu, (cr >> (8u - ush)) & 0xffu, kc), kc);
        };
        auto math = [&](int j) {
            unsigned l0[4], r0w[4], l1[4], r1w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                taps(ya0[j][k], ca0[j][k], ro0[j] + xo[k], co0[j] + xc[k], st[k], l0[k], r0w[k]);
                taps(ya1[j][k], ca1[j][k], ro1[j] + xo[k], co1[j] + xc[k], st[k], l1[k], r1w[k]);
            }
            finish(j, l0, r0w, l1, r1w, byw0[j], byw1[j]);
        };
#pragma unroll
        for (int h = 0; h < IPT; h += HS) {
#pragma unroll
            for (int j = 0; j < HS; ++j) issue(h + j);
#pragma unroll
            for (int j = 0; j < HS; ++j) math(h + j);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    // P010 (also P016): NV12 with 16-bit little-endian samples of which the high byte counts.  The column entries point at the high
    // bytes (yuv_layout: luma at 2 x + 1), so a tap pair's luma is bytes 0 and 2 of a 3-byte window: the aligned 8 bytes that hold its
    // first byte cover it (first byte at 1 or 3 of them).  Its one or two chroma pairs are 8 bytes (Ulo Uhi Vlo Vhi, twice) at any
    // alignment (pitch1 may be odd): the 12 aligned bytes that hold them, two funnel shifts, U and V at bytes 1 and 3 of each dword.
    // One item at a time: the chroma windows are three registers, and two items' windows do not fit the 128 registers of the others.
    // GUARD, re-derived for these widths (x <= W - 2, y <= H - 2 always: the crop's valid range stops one short):
    //   luma: the window's first byte is at o <= pitch0 y + 2 (W - 2) + 1; its aligned 8 bytes end before o + 8 <= pitch0 y + 2 W + 5,
    //     inside the plane [0, pitch0 (H - 1) + 2 W) for y <= H - 2 as pitch0 >= 2 W >= 4 (the chroma condition below covers it anyway)
    //   chroma: the pairs start at o <= pitch1 (y >> 1) + 2 W - 4; their aligned 12 bytes end before o + 12 <= pitch1 (y >> 1) + 2 W + 8:
    //     inside [0, pitch1 (H / 2 - 1) + 2 W) when y >> 1 <= H / 2 - 2 and pitch1 >= 8, and up to 8 bytes past it in the LAST chroma row
    //     (y = H - 2).  So a band whose valid source rows reach H - 2, or a plane narrower than 8 bytes, takes the guarded form.
    auto p010 = [&](auto guard_c) {
        constexpr bool GUARD = decltype(guard_c)::value;
        auto load8 = [&](unsigned o) -> u2v {
            const unsigned a = o & ~3u;
            if (!GUARD || a + 8u <= iv.nrec0) return __builtin_amdgcn_raw_buffer_load_b64(rs0, (int)a, 0, 0);
            unsigned w[2] = {0u, 0u};
#pragma unroll
            for (int i = 0; i < 8; ++i) w[i >> 2] |= ((unsigned)__builtin_amdgcn_raw_buffer_load_b8(rs0, (int)(a + i), 0, 0) & 0xffu) << (8 * (i & 3));
            return u2v{w[0], w[1]};
        };
        auto load12 = [&](unsigned o) -> u3v {
            const unsigned a = o & ~3u;
            if (!GUARD || a + 12u <= iv.nrec1) return __builtin_amdgcn_raw_buffer_load_b96(rs1, (int)a, 0, 0);
            unsigned w[3] = {0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < 12; ++i) w[i >> 2] |= ((unsigned)__builtin_amdgcn_raw_buffer_load_b8(rs1, (int)(a + i), 0, 0) & 0xffu) << (8 * (i & 3));
            return u3v{w[0], w[1], w[2]};
        };
        auto taps = [&](const u2v& yw, const u3v& cw, unsigned yo, unsigned co, unsigned s, unsigned& l, unsigned& r) {
            const unsigned y = __builtin_amdgcn_alignbit(yw.y, yw.x, yo << 3);      // the left tap's luma at byte 0, the next pixel's at byte 2
            const unsigned cl = __builtin_amdgcn_alignbit(cw.y, cw.x, co << 3);     // the left tap's pair: U at byte 1, V at byte 3
            const unsigned cr = (s & 2u) ? __builtin_amdgcn_alignbit(cw.z, cw.y, co << 3) : cl;
            l = yuv_rgb(y & 0xffu, chroma_terms((cl >> 8) & 0xffu, cl >> 24, kc), kc);
            r = yuv_rgb((s & 1u) ? (y >> 16) & 0xffu : y & 0xffu, chroma_terms((cr >> 8) & 0xffu, cr >> 24, kc), kc);
        };
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            const u4v e = *reinterpret_cast<const u4v*>(ytab + 4 * (j * RPG + rl));
            const u2v cr = *reinterpret_cast<const u2v*>(ctab + 2 * (j * RPG + rl));
            const bool live = ((e.z | e.w) != 0u) && col_live;
            u2v ya0[4], ya1[4];
            u3v ca0[4], ca1[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!live) {
                    ya0[k] = u2v{0u, 0u}; ya1[k] = u2v{0u, 0u}; ca0[k] = u3v{0u, 0u, 0u}; ca1[k] = u3v{0u, 0u, 0u};
                    continue;
                }
                ya0[k] = load8(e.x + xo[k]);
                ya1[k] = load8(e.y + xo[k]);
                ca0[k] = load12(cr.x + xc[k]);
                ca1[k] = load12(cr.y + xc[k]);
            }
            unsigned l0[4], r0w[4], l1[4], r1w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                taps(ya0[k], ca0[k], e.x + xo[k], cr.x + xc[k], st[k], l0[k], r0w[k]);
                taps(ya1[k], ca1[k], e.y + xo[k], cr.y + xc[k], st[k], l1[k], r1w[k]);
            }
            finish(j, l0, r0w, l1, r1w, e.z, e.w);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    // I420 / YV12, YUYV / UYVY, GRAY8, I444 / I422, RGBP / BGRP: the band's tables, every sample of a tap fetched as a single byte through
    // the bounded descriptors (yuv_layout says where: the two chroma planes of I420 / I444 / I422 are plane 1 at offsets 0 and p2, packed
    // 4:2:2 keeps its chroma in plane 0; planar RGB lies as I444 does and skips the conversion).
    // Every offset lies inside its plane by construction (x + step <= W - 1, rows <= H - 2): no guard form.
    // PRGB: planar RGB, an instantiation of its own, so that the loop of the layouts that were here first compiles as it did.
    // The wide family's byte layouts (YV16 / YV24, NV16 / NV24, P210 / P410, the 16-bit planar ones through their high bytes) are rows
    // of yuv_layout and run this loop as it is.
    // WIDE: the 10- and 12-bit planar layouts and GRAY10 / GRAY12, an instantiation of its own: every sample ONE 16-bit load through the
    // same bounded descriptors, s8 = min(word >> wsh, 255) with wsh = depth - 8 uniform, then this loop -- as many loads as the byte
    // family issues.  Bound: image_view admits these layouts at even plane addresses and even pitches only, the column entries are
    // 2 x (yadd = 0) and 2 (x >> cxs), the trailing plane begins at the even p2: every word's offset is even, and the extent
    // pitch (rows - 1) + 2 (samples a row) is even too, so the last word starts at extent - 2 -- no load starts at the extent's last
    // byte or crosses it.
    auto bytewise = [&](auto prgb_c, auto wide_c) {
        constexpr bool PRGB = decltype(prgb_c)::value, WIDE = decltype(wide_c)::value;
        const bool gray = is_gray_layout(fmt), pbgr = fmt == VT_PIX_BGRP;
        const unsigned ystep = yl.ymul, cstepb = yl.cmul;
        const unsigned wsh = wide_shift(fmt);
        auto s8 = [&](unsigned w) { w = (w & 0xffffu) >> wsh; return w < 255u ? w : 255u; };
        auto lum = [&](unsigned o) {
            if constexpr (WIDE) return s8((unsigned)__builtin_amdgcn_raw_buffer_load_b16(rs0, (int)o, 0, 0));
            else return (unsigned)__builtin_amdgcn_raw_buffer_load_b8(rs0, (int)o, 0, 0) & 0xffu;
        };
        auto chr = [&](unsigned o) {
            if constexpr (WIDE) return s8((unsigned)__builtin_amdgcn_raw_buffer_load_b16(rs1, (int)o, 0, 0));
            else return (unsigned)__builtin_amdgcn_raw_buffer_load_b8(rs1, (int)o, 0, 0) & 0xffu;
        };
        auto tap = [&](unsigned yo, unsigned co) -> unsigned {
            if constexpr (PRGB) {
                return planar_rgb(lum(yo), chr(co + yl.uoff), chr(co + yl.voff), pbgr);
            } else {
                if (gray) return lum(yo) * 0x010101u;
                const unsigned u = chr(co + yl.uoff), v = chr(co + yl.voff);
                return yuv_rgb(lum(yo), chroma_terms(u, v, kc), kc);
            }
        };
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            const u4v e = *reinterpret_cast<const u4v*>(ytab + 4 * (j * RPG + rl));
            const u2v cr = *reinterpret_cast<const u2v*>(ctab + 2 * (j * RPG + rl));
            const bool live = ((e.z | e.w) != 0u) && col_live;
            unsigned l0[4], r0w[4], l1[4], r1w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!live) { l0[k] = 0u; r0w[k] = 0u; l1[k] = 0u; r1w[k] = 0u; continue; }
                const unsigned ys = (st[k] & 1u) ? ystep : 0u, cs = (st[k] & 2u) ? cstepb : 0u;
                l0[k] = tap(e.x + xo[k], cr.x + xc[k]);
                r0w[k] = tap(e.x + xo[k] + ys, cr.x + xc[k] + cs);
                l1[k] = tap(e.y + xo[k], cr.y + xc[k]);
                r1w[k] = tap(e.y + xo[k] + ys, cr.y + xc[k] + cs);
            }
            finish(j, l0, r0w, l1, r1w, e.z, e.w);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    if (nv || fmt == VT_PIX_P010) {
        // the guard: a band whose valid source rows reach row H - 2 reads the last chroma row; planes narrower than 8 bytes
        const int ymax = band_last_source_row<NROWS>(row0, g);
        const bool guard = ymax >= iv.H - 2 || iv.pitch0 < 8u || iv.pitch1 < 8u;
        if (!nv) {
            if (guard) p010(std::true_type{});
            else p010(std::false_type{});
        } else {      // NV12 / NV21 under one of the three other colour rows (BT.601 limited never comes here)
            if (guard) yuv(std::true_type{});
            else yuv(std::false_type{});
        }
    } else if (is_planar_rgb(fmt)) {
        bytewise(std::true_type{}, std::false_type{});
    } else if (wide_shift(fmt) != 0u) {
        bytewise(std::false_type{}, std::true_type{});
    } else {
        bytewise(std::false_type{}, std::false_type{});
    }
}

// crop_band_image_kernel: crop_band_kernel on a vt_image table (T = 64 / 128 / 256, the tracker's per-step crop), same bands, tables,
// arithmetic and results.  The format is uniform in a workgroup (one workgroup crops one sequence), so each format family is its own
// instantiation of the body inside one kernel, picked by a uniform branch; a table may still mix formats.
//   - packed (RGB / BGR: 3 bytes, RGBA / BGRA: 4 bytes a pixel): a window of two pixels is fetched as the 12 ALIGNED bytes that contain
//     it and funnel-shifted into place, as crop_band_kernel's aligned form.  The order of the channels is the byte select of the
//     v_perm_b32 that already picks a channel out of the window: BGR costs nothing.
//   - NV12 / NV21: a tap pair reads its two luma bytes as the aligned 8 bytes that hold them, and its one or two chroma pairs as the
//     aligned 8 bytes that hold them; each tap is converted to RGB in int32, then the same 11-bit bilinear code.
//   - bounds: the crop never reads the last row or column of a frame (its valid range stops one short: see crop_kernel), so the packed
//     windows and the luma windows stay inside their plane (pitch >= 8); a chroma window of the LAST chroma row can overhang its plane
//     by up to 6 bytes: a band that reads that row (or a plane narrower than 8 bytes) takes the GUARD form, where a window that would
//     cross its plane's end is read as single bytes.  The buffer descriptors bound every load to its plane's extent regardless.
template <bool U8OUT, int LGT4, int IPT>
__global__ __launch_bounds__(256) void crop_band_image_kernel(const vt_image* __restrict__ images, vt_frame* __restrict__ sizes,
                                                              const double* __restrict__ states, double factor,
                                                              float m0, float m1, float m2, float s0, float s1, float s2,
                                                              float* __restrict__ out, double* __restrict__ resize_factor) {
    constexpr int T4 = 1 << LGT4, T = 4 * T4, RPG = 256 >> LGT4, NROWS = IPT * RPG;
    static_assert(T <= 256 && (T * T4) % (IPT * 256) == 0, "a band is whole rows and the frame whole bands");
    const int b = blockIdx.y, tid = threadIdx.x;
    // a format word beyond the six first layouts -- another layout, or colour bits -- is cropped by crop_band_image_ext (above); the code
    // below is, to the instruction, what cropped those six before the others existed, and they pay one scalar compare for them
    if ((unsigned)images[b].format > (unsigned)VT_PIX_NV21) {
        crop_band_image_ext<U8OUT, LGT4, IPT>(images, sizes, states, factor, m0, m1, m2, s0, s1, s2, out, resize_factor);
        return;
    }
    const ImageView6 iv = image_view6(images, b);
    __shared__ float norm_lut[U8OUT ? 1 : 3 * 256];
    __shared__ __attribute__((aligned(16))) unsigned xtab[T * 4];          // per output column: plane-0 byte offset of the window, packed weights, steps, chroma offset
    __shared__ __attribute__((aligned(16))) unsigned ytab[NROWS * 4];      // per output row: plane-0 offsets of its two source rows, their weights << 12
    __shared__ __attribute__((aligned(8))) unsigned ctab[NROWS * 2];       // per output row: chroma-row offsets of its two source rows (NV12 / NV21)
    unsigned char* const out8 = reinterpret_cast<unsigned char*>(out) + (size_t)b * T * T * 3;
    if constexpr (!U8OUT) fill_norm_lut(norm_lut, m0, m1, m2, s0, s1, s2);
    const int crop_sz = crop_side(states, b, factor);
    const int row0 = blockIdx.x * NROWS;
    const int cg = tid & (T4 - 1), rl = tid >> LGT4;
    if (blockIdx.x == 0 && tid == 0) image_sizes_out(sizes, images, b);
    if (!(crop_sz >= 1) || !iv.ok) {        // see poison_item
        poison_band<U8OUT, T, IPT, RPG>(out, out8, resize_factor, b, row0, rl, cg);
        return;
    }
    const int fmt = iv.fmt;
    const bool nv = fmt == VT_PIX_NV12 || fmt == VT_PIX_NV21, four = fmt == VT_PIX_RGBA || fmt == VT_PIX_BGRA;
    const unsigned bpp = nv ? 1u : (four ? 4u : 3u);
    const CropWindow g = crop_window(states, b, crop_sz, T, iv.H, iv.W);
    if (blockIdx.x == 0 && tid == 0) resize_factor[b] = (double)T / (double)crop_sz;
    fill_band_tables<T, NROWS>(xtab, ytab, ctab, row0, g, iv.pitch0, 1u, iv.pitch1,
                               [&](const ColumnTap& t) { return image_column_entry(t, bpp, 0u, 2u); });
    __syncthreads();
    const auto rs0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(iv.p0), 0, (int)iv.nrec0, 0x00020000);
    const auto rs1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(nv ? iv.p1 : iv.p0), 0, (int)iv.nrec1, 0x00020000);
    unsigned xo[4], wp[4], st[4], xc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const u4v e = *reinterpret_cast<const u4v*>(xtab + 4 * (4 * cg + k));
        xo[k] = e.x; wp[k] = e.y; st[k] = e.z; xc[k] = e.w;
    }
    // the byte of each channel in an RGB-ordered (or, swapped, BGR-ordered) pixel dword: v_perm_b32 selectors
    // [left pixel's channel, 0, right pixel's channel, 0], uniform
    const bool swap = fmt == VT_PIX_BGR || fmt == VT_PIX_BGRA;
    unsigned sel[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) sel[c] = 0x0c040c00u + 0x00010001u * (unsigned)(swap ? 2 - c : c);
    const unsigned ush = fmt == VT_PIX_NV21 ? 8u : 0u;      // bit offset of U in a chroma pair (V at the other byte)
    unsigned two = 2u;
    asm volatile("" : "+v"(two));
    const bool col_live = (wp[0] | wp[1] | wp[2] | wp[3]) != 0u;
    // the output of one item from its four tap-pair dwords per row (l = left tap, r = right tap: R | G << 8 | B << 16)
    // item 7: not merged, see NOTES.md (crop kernels)
    auto finish = [&](int j, const unsigned (&l0)[4], const unsigned (&r0w)[4], const unsigned (&l1)[4], const unsigned (&r1w)[4],
                      unsigned byw0, unsigned byw1) {
        const int oy = row0 + j * RPG + rl;
        float res[3][4];
        unsigned pk[3] = {0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const us2 wv = __builtin_bit_cast(us2, wp[k]);
#pragma unroll
            for (int c = 0; c < 3; ++c) {       // crop_band_kernel's arithmetic
                const unsigned r0 = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, __builtin_amdgcn_perm(r0w[k], l0[k], sel[c])), wv, 0u, false);
                const unsigned r1 = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, __builtin_amdgcn_perm(r1w[k], l1[k], sel[c])), wv, 0u, false);
                const unsigned t0 = mulhi24(byw0, r0 & ~15u), t1 = mulhi24(byw1, r1 & ~15u);
                if constexpr (U8OUT) {
                    put_byte_shr2(pk[(3 * k + c) >> 2], t0 + t1 + 2u, two, (3 * k + c) & 3);
                } else {
                    const unsigned v4 = (t0 + t1 + 2u) & ~3u;
                    res[c][k] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(norm_lut) + c * 1024 + v4);
                }
            }
        }
        if constexpr (U8OUT) {
            *reinterpret_cast<u3a*>(out8 + ((size_t)oy * T + 4 * cg) * 3) = u3a{pk[0], pk[1], pk[2]};
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) st4(out + (((size_t)b * 3 + c) * T + oy) * T + 4 * cg, f4{res[c][0], res[c][1], res[c][2], res[c][3]});
        }
    };
    constexpr int HS = IPT < 2 ? IPT : 2;      // two items at a time, as crop_band_kernel
    // packed formats: BPP 3 or 4
    // item 8: not merged, see NOTES.md (crop kernels)
    auto packed = [&](auto bpp_c) {
        constexpr unsigned BPP = decltype(bpp_c)::value;
        u3v ra0[IPT][4], ra1[IPT][4];
        unsigned ro0[IPT], ro1[IPT], byw0[IPT], byw1[IPT];
        auto issue = [&](int j) {
            const u4v e = *reinterpret_cast<const u4v*>(ytab + 4 * (j * RPG + rl));
            ro0[j] = e.x; ro1[j] = e.y; byw0[j] = e.z; byw1[j] = e.w;
            const bool live = ((e.z | e.w) != 0u) && col_live;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!live) { ra0[j][k] = u3v{0u, 0u, 0u}; ra1[j][k] = u3v{0u, 0u, 0u}; continue; }
                ra0[j][k] = __builtin_amdgcn_raw_buffer_load_b96(rs0, (int)((e.x + xo[k]) & ~3u), 0, 0);
                ra1[j][k] = __builtin_amdgcn_raw_buffer_load_b96(rs0, (int)((e.y + xo[k]) & ~3u), 0, 0);
            }
        };
        auto math = [&](int j) {
            unsigned l0[4], r0w[4], l1[4], r1w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned b0 = (ro0[j] + xo[k]) << 3, b1 = (ro1[j] + xo[k]) << 3;      // v_alignbit reads bits [4:0]: 8 x (offset & 3)
                const u2v w0{__builtin_amdgcn_alignbit(ra0[j][k].y, ra0[j][k].x, b0), __builtin_amdgcn_alignbit(ra0[j][k].z, ra0[j][k].y, b0)};
                const u2v w1{__builtin_amdgcn_alignbit(ra1[j][k].y, ra1[j][k].x, b1), __builtin_amdgcn_alignbit(ra1[j][k].z, ra1[j][k].y, b1)};
                l0[k] = w0.x; l1[k] = w1.x;
                if constexpr (BPP == 3) {
                    r0w[k] = (st[k] & 1u) ? __builtin_amdgcn_alignbit(w0.y, w0.x, 24u) : w0.x;
                    r1w[k] = (st[k] & 1u) ? __builtin_amdgcn_alignbit(w1.y, w1.x, 24u) : w1.x;
                } else {
                    r0w[k] = (st[k] & 1u) ? w0.y : w0.x;
                    r1w[k] = (st[k] & 1u) ? w1.y : w1.x;
                }
            }
            finish(j, l0, r0w, l1, r1w, byw0[j], byw1[j]);
        };
#pragma unroll
        for (int h = 0; h < IPT; h += HS) {
#pragma unroll
            for (int j = 0; j < HS; ++j) issue(h + j);
#pragma unroll
            for (int j = 0; j < HS; ++j) math(h + j);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    // NV12 / NV21; GUARD: windows that would cross their plane's end are read as single bytes
    // items 9 and 8: not merged, see NOTES.md (crop kernels)
    auto yuv = [&](auto guard_c) {
        constexpr bool GUARD = decltype(guard_c)::value;
        u2v ya0[IPT][4], ya1[IPT][4], ca0[IPT][4], ca1[IPT][4];
        unsigned ro0[IPT], ro1[IPT], co0[IPT], co1[IPT], byw0[IPT], byw1[IPT];
        auto load8 = [&](const auto& rs, unsigned o, unsigned nrec) -> u2v {      // the 8 bytes from the dword that holds byte o
            const unsigned a = o & ~3u;
            if (!GUARD || a + 8u <= nrec) return __builtin_amdgcn_raw_buffer_load_b64(rs, (int)a, 0, 0);
            unsigned lo = 0u, hi = 0u;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                lo |= ((unsigned)__builtin_amdgcn_raw_buffer_load_b8(rs, (int)(a + i), 0, 0) & 0xffu) << (8 * i);
                hi |= ((unsigned)__builtin_amdgcn_raw_buffer_load_b8(rs, (int)(a + 4 + i), 0, 0) & 0xffu) << (8 * i);
            }
            return u2v{lo, hi};
        };
        auto issue = [&](int j) {
            const u4v e = *reinterpret_cast<const u4v*>(ytab + 4 * (j * RPG + rl));
            const u2v cr = *reinterpret_cast<const u2v*>(ctab + 2 * (j * RPG + rl));
            ro0[j] = e.x; ro1[j] = e.y; byw0[j] = e.z; byw1[j] = e.w; co0[j] = cr.x; co1[j] = cr.y;
            const bool live = ((e.z | e.w) != 0u) && col_live;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!live) {      // (one assignment each: chained, they kept the arrays in scratch)
                    ya0[j][k] = u2v{0u, 0u}; ya1[j][k] = u2v{0u, 0u}; ca0[j][k] = u2v{0u, 0u}; ca1[j][k] = u2v{0u, 0u};
                    continue;
                }
                ya0[j][k] = load8(rs0, e.x + xo[k], iv.nrec0);
                ya1[j][k] = load8(rs0, e.y + xo[k], iv.nrec0);
                ca0[j][k] = load8(rs1, cr.x + xc[k], iv.nrec1);
                ca1[j][k] = load8(rs1, cr.y + xc[k], iv.nrec1);
            }
        };
        auto taps = [&](const u2v& yw, const u2v& cw, unsigned yo, unsigned co, unsigned s, unsigned& l, unsigned& r) {
            const unsigned y = __builtin_amdgcn_alignbit(yw.y, yw.x, yo << 3);      // luma of the left tap at byte 0, the next pixel's at byte 1
            const unsigned c = __builtin_amdgcn_alignbit(cw.y, cw.x, co << 3);      // the left tap's chroma pair at bytes 0-1, the next pair at 2-3
            const unsigned cl = c & 0xffffu, cr = (s & 2u) ? c >> 16 : cl;
            l = yuv_rgb(y & 0xffu, chroma_terms((cl >> ush) & 0xffu, (cl >> (8u - ush)) & 0xffu));
            r = yuv_rgb((s & 1u) ? (y >> 8) & 0xffu : y & 0xffu, chroma_terms((cr >> ush) & 0xffu, (cr >> (8u - ush)) & 0xffu));
        };
        auto math = [&](int j) {
            unsigned l0[4], r0w[4], l1[4], r1w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                taps(ya0[j][k], ca0[j][k], ro0[j] + xo[k], co0[j] + xc[k], st[k], l0[k], r0w[k]);
                taps(ya1[j][k], ca1[j][k], ro1[j] + xo[k], co1[j] + xc[k], st[k], l1[k], r1w[k]);
            }
            finish(j, l0, r0w, l1, r1w, byw0[j], byw1[j]);
        };
#pragma unroll
        for (int h = 0; h < IPT; h += HS) {
#pragma unroll
            for (int j = 0; j < HS; ++j) issue(h + j);
#pragma unroll
            for (int j = 0; j < HS; ++j) math(h + j);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    if (nv) {
        // the guard: a band whose valid source rows reach row H - 2 reads the last chroma row; planes narrower than 8 bytes
        const int ymax = band_last_source_row<NROWS>(row0, g);
        if (ymax >= iv.H - 2 || iv.pitch0 < 8u || iv.pitch1 < 8u) yuv(std::true_type{});
        else yuv(std::false_type{});
    } else if (four) {
        packed(std::integral_constant<unsigned, 4>{});
    } else {
        packed(std::integral_constant<unsigned, 3>{});
    }
}

// One thread per sequence.  hann_boxes (B,4) float [cx,cy,w,h] in [0,1]; states (B,4) double in/out.
// `record` (optional, (B,5) double, device memory or device-mapped pinned host memory): [x, y, w, h, confidence] of the new state --
// what track() returns; written here, the step needs no copy kernel and no device -> host copy after it.
__global__ void update_state_kernel(const float* __restrict__ hann_boxes, const double* __restrict__ resize_factor,
                                    int search_size, int H, int W, int margin, int B, double* __restrict__ states,
                                    const float* __restrict__ conf, double* __restrict__ record) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float hb[4] = {hann_boxes[4 * b + 0], hann_boxes[4 * b + 1], hann_boxes[4 * b + 2], hann_boxes[4 * b + 3]};
    const TrackTail t{resize_factor, states, record, search_size, H, W, margin, 0};
    update_state_one(b, hb, conf != nullptr ? conf[b] : 0.f, t);
}

}  // namespace vtt

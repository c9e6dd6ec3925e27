// vittrack.hip -- C-ABI runtime of libvittrack_hip.so (see include/vittrack.h).
// Host side, in this order: switches (read_switches), kernel forms (the tables and selectors: the ONE place where a form is chosen),
// the step (vt48_network, vitb_network, fork_join), crop front end, model set-up, ABI.  Weight folding and packing: vt_weights.h.
// Device side: vt_stem*.h / vt_blocks*.h / vt_head*.h / vt_track.h / vt_generic.h.
#include "../../include/vittrack.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "vb_api.h"
#include "vt_blocks.h"
#include "vt_blocks_tile.h"
#include "vt_head.h"
#ifndef VT_SEQ3_MAXP
#define VT_SEQ3_MAXP 2      // head_seq3: conv1 weight pairs per register pass
#endif
#include "vt_head3.h"
#include "vt_generic.h"
#include "vt_stem.h"
#include "vt_stem_fused.h"
#include "vt_stem_stream.h"
#include "vt_track.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess)                                                                     \
            return fail(VT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));           \
    } while (0)

struct DevBuf {
    float* p = nullptr;
    size_t n = 0;
    int alloc(size_t floats) {
        n = floats;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), floats * sizeof(float));
        if (e != hipSuccess) return fail(VT_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
        return VT_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
};

constexpr int STEM_CH[5] = {3, 6, 12, 24, 48};

// dynamic LDS of blocks_kernel<NT, ., ., WLDS, BAL, ., BF3, A3> at a given depth: K/V images, weight staging buffers,
// the small parameters (LayerNorm vectors + biases of every block) and the guests' exchange area
size_t blocks_lds_bytes(int NT, bool WLDS, bool BAL, int depth, bool BF3 = false, bool A3 = false) {
    if (A3 && !WLDS)    // the G256 form: K as pieces, V^T an fp32 image, no staging buffers, no guests
        return ((size_t)NT * vtb::W3_FC1_OT16 + (size_t)vtb::NC * NT * 64) * sizeof(f4) + (size_t)vtb::small_floats(depth) * sizeof(float);
    if (A3)     // K / V^T as pieces (vt_blocks.h: KV_UNITS); of the guests' areas only Dg and the counter keep room of their own
        return ((size_t)NT * vtb::W3_FC1_OT16 + (size_t)vtb::NC * ((NT / 2) * 3 * 64 + (NT & 1) * 3 * 32) +
                (size_t)(vtb::W3_FC1_TILES + vtb::WBUF_TILES) * 64) * sizeof(f4) +
               (size_t)vtb::small_floats(depth) * sizeof(float) + (size_t)vtb::NC * 64 * sizeof(f4) + 64;
    return ((size_t)2 * NT * vtb::NC + (WLDS ? (BF3 ? vtb::W3_FC1_TILES : vtb::WBUF_TILES) + vtb::WBUF_TILES : 0)) * 64 * sizeof(f4) +
           (size_t)vtb::small_floats(depth) * sizeof(float) +
           (BAL ? (size_t)(vtb::NC + 4 * vtb::NC + vtb::NC) * 64 * sizeof(f4) + 4 * 2 * 64 * sizeof(float) + 64 : 0);
}
constexpr size_t LDS_PER_CU = 160 * 1024;

// ------------------------------------------------------------------------------------- switches
// The only two functions that look at the environment; read_switches, crop_switches and stem_plan go through them.
bool env_set(const char* name) {
    const char* v = std::getenv(name);
    return v && *v;
}
int env_int(const char* name, int dflt) { return env_set(name) ? std::atoi(std::getenv(name)) : dflt; }

// Every VT_* variable a model reads, read ONCE at vt_create by read_switches; the diagnostic ones are 0 / -1 in production.
// Kernel form per stage: 1 / 0 force it, -1 (default) = by batch size.  The one-workgroup-per-frame forms win once the batch
// fills the chip; below that the multi-workgroup forms spread a frame over several CUs (measured, us per step, tools/
// small_batch_sweep.py: G128 B=1 97.6 -> 81.1, B=64 100.4 -> 86.1; G256 B=1 337 -> 287; crossovers at the thresholds of the selectors).
struct Switches {
    int skip_stem_a = 0, skip_stem_b = 0, skip_head = 0, dbg_skip_tile = -1;   // timing diagnostics, wrong results by design
    int dbg_stamps = 0;    // VT_DBG_STAMPS=1: per-wave phase stamps of the block kernel (vt_debug_stamps)
    int track_u8 = 1;      // VT_TRACK_U8: vt_track_step hands the crop to the stem as a uint8 patch (0: the fp32 crop of vt_crop)
    int graph_chains = 1, chain_cus = 0, chain_delay_us = 0;   // graph chains: see read_switches
    int head_fused = -1;   // F = 8: head_fused_kernel (towers + decode in one workgroup per frame); auto: B > 176
                           // F = 16: head_seq_kernel (one workgroup per frame runs the three towers in turn, then decodes); auto: B > 176
    int head_bf3 = 1;      // VT_HEAD_BF3: the towers on the bf16 matrix pipe at fp32 accuracy (F = 8); 0 = fp32 MFMA towers
    int head_split = -1;   // F = 16: conv1 as a launch of its own over row strips (1 / 0 force, -1: by batch size)
    int stem_pipe = -1;    // G256: stem_pipe_kernel (layers 1 + 2 per frame) instead of stem_a; auto: B > 176
    int stem_fused = -1;   // G128: stem_fused_kernel (one workgroup per frame) instead of stem_a + stem_b; auto: B > 80
    int stem_stream = -1;  // stem_stream_kernel (all four layers of a frame streamed band by band through one workgroup) instead of
                           // stem_pipe + stem_b (G256) / stem_fused (G128); auto: G256 B > 176 (fp32 build)
    int stem_fuse = 1;     // stem_a: one workgroup = band k of both crops (G128: 4 instead of 5 workgroups per frame)
    int stem_bf3 = 1;      // VT_STEM_BF3: layer 3 of stem_fused as exact three-piece bf16 products (fp32 build); 0 = fp32 MFMAs
    bool r4_128_forced = false;   // VT_STEM_R4_128 was set: keep that band height at every batch size
    int blocks_tile = -1;  // 1 / 0 force the tile-parallel form of the blocks / forbid it, -1 (default): by batch size
    int blocks_bf3 = 2;    // VT_BLOCKS_BF3: the G128 frame form's contractions as exact three-piece bf16 products: 2 = all of them
                           // (A3: attention + proj too), 1 = qkv + MLP, 0 = fp32 MFMAs
    int blocks_bf3_g256 = 2;   // the same switch at G256 (1: MLP only, weights from L2)
    int blocks_bal = 1;    // G128 block kernel: balanced 4 owner + 4 guest waves (1) or one wave per tile (0)
    int blocks_wlds = 1;   // G128 block kernel: weights staged through LDS (1) or read from L2 per wave (0)
};

Switches read_switches(const vt_config& cfg, bool vitb) {
    Switches s;
    s.skip_stem_a = env_int("VT_SKIP_STEM_A", 0);
    s.skip_stem_b = env_int("VT_SKIP_STEM_B", 0);
    s.skip_head = env_int("VT_SKIP_HEAD", 0);
    s.dbg_skip_tile = env_int("VT_DBG_SKIP_TILE", -1);
    s.dbg_stamps = env_int("VT_DBG_STAMPS", 0);
    s.track_u8 = env_int("VT_TRACK_U8", 1);
    // graph chains (vt_graph_capture_steps, the ViT-Base tracker step): frame slices of one step as concurrent chains.  vit_48: one chain
    // unless asked.  ViT-Base default (round 5; 0 = auto): a step of >= 64 frames runs as TWO chains of half the frames whose persistent
    // GEMMs each launch a workgroup per CU -- the chains' kernels then fill each other's last, partly empty tile rounds (3.75 of 4, 7.5
    // of 8 at B = 256) and ramps: 17.63 -> 16.88 ms per step at B = 256 (tools/gpu_vbchains.sh; each chain on HALF the CUs instead:
    // 17.66, i.e. nothing -- NOTES R5-6).  Frames are independent: outputs are bit-identical to the one-chain step
    // (tests/test_gpu_variants.py).  VT_CHAIN_CUS / VT_CHAIN_DELAY_US have only ever been read for ViT-Base models.
    s.graph_chains = env_int("VT_GRAPH_CHAINS", vitb ? 0 : 1);
    if (vitb) {
        s.chain_cus = env_int("VT_CHAIN_CUS", 0);
        s.chain_delay_us = env_int("VT_CHAIN_DELAY_US", 0);
    }
    s.blocks_wlds = env_int("VT_BLOCKS_WLDS", 1);
    s.blocks_bal = env_int("VT_BLOCKS_BAL", 1);
    s.blocks_bf3 = s.blocks_bf3_g256 = env_int("VT_BLOCKS_BF3", 2);
    if (s.blocks_bf3_g256 >= 2 && blocks_lds_bytes(20, false, false, cfg.depth, true, true) > LDS_PER_CU) s.blocks_bf3_g256 = 1;
    if (s.blocks_bf3 >= 2 && blocks_lds_bytes(5, true, true, cfg.depth, true, true) > LDS_PER_CU) s.blocks_bf3 = 1;
    // the BF3 form's staging buffers are 18 KiB larger: beyond depth 8 its small parameters no longer fit beside them -> fp32 form
    if (blocks_lds_bytes(5, true, true, cfg.depth, true) > LDS_PER_CU) s.blocks_bf3 = 0;
    s.stem_fused = env_int("VT_STEM_FUSED", -1);
    s.stem_pipe = env_int("VT_STEM_PIPE", -1);
    s.stem_stream = env_int("VT_STEM_STREAM", -1);
    s.head_fused = env_int("VT_HEAD_FUSED", -1);
    s.head_bf3 = env_int("VT_HEAD_BF3", 1);      // default since the sustained A/B (tools/power_probe.py): 93.5 -> 86.4 us per step at equal clocks
    s.blocks_tile = env_int("VT_BLOCKS_TILE", -1);
    s.head_split = env_int("VT_HEAD_SPLIT", -1);
    s.stem_fuse = env_int("VT_STEM_FUSE", cfg.search_size == 128 ? 1 : 0);
    s.stem_bf3 = env_int("VT_STEM_BF3", 1);
    s.r4_128_forced = env_set("VT_STEM_R4_128");
    return s;
}

// The process-wide crop switches: read once, at the first crop (or crop self test) of the process.
struct CropSwitches {
    int fast = 1;        // VT_CROP_FAST: groups per workgroup of crop_fast_kernel (1, 2, 4); 0: crop_kernel
    int band = 4;        // VT_CROP_BAND: crop_band_kernel, a workgroup owns a band of VT_CROP_BAND x 256 items (0: crop_fast_kernel as in
                         // round 5; -4 / -2 force a band form at any batch: tests)
    bool band_set = false;   // VT_CROP_BAND was given: it decides for the fp32 form too (crop_band_ipt)
    int aligned = 1;     // VT_CROP_ALIGNED: 0 = byte-aligned 8-byte windows
    int bytes = -1;      // VT_CROP_BYTES: force the byte-load form (1) or the fast form (0) whatever the self test finds (tests); -1: unset
};
const CropSwitches& crop_switches() {
    static const CropSwitches s = [] {
        CropSwitches c;
        c.fast = env_int("VT_CROP_FAST", 1);
        c.band = env_int("VT_CROP_BAND", 4);
        c.band_set = env_set("VT_CROP_BAND");
        c.aligned = env_int("VT_CROP_ALIGNED", 1);
        if (env_set("VT_CROP_BYTES")) c.bytes = env_int("VT_CROP_BYTES", 0) != 0 ? 1 : 0;
        return c;
    }();
    return s;
}

}  // namespace

struct vt_model {
    VbModel* vb = nullptr;           // ViT-Base / ViT-Large path (channels = 768 / 1024): backbone + head towers live in vitb.hip
    // any other stride-16 geometry of the vit_48_h32 surface: the shape-generic kernels of vt_generic.h
    bool generic = false;
    vtg::Dims gd{48, 1, 32};         // widths of the shape-generic path (round 6: any CHANNELS / HEADS / HEAD.NUM_CHANNELS)
    DevBuf g_stem_w[4], g_stem_b[4]; // folded conv weights [cout][cin][9] / bias
    DevBuf g_blocks;                 // depth * gd.block_stride() + 2 C (final norm)
    DevBuf g_head;                   // 3 * gd.tower_stride()
    DevBuf g_a, g_b;                 // stem ping-pong maps; then the head's
    DevBuf g_qkv, g_ao, g_hid, g_x;  // (B L, 3 C), (B L, C), (B L, 4 C); the residual stream being updated
    vt_config cfg{};
    Switches sw;                     // the VT_* variables, as read at vt_create
    int len_z = 0, len_x = 0, L = 0, F = 0, Fz = 0;
    bool weights_loaded = false;
    // parameters on the device
    DevBuf stem_w[4], stem_b[4];     // folded, [group][tap][cin][OCG] / [cout]
    DevBuf stem_w3b;                 // layer 3 as three-piece bf16 images (stem_fused, fp32 build)
    DevBuf stem_w4b;                 // layer 4, the same way: [out tile 3][chunk pair 7][piece 3][64 lanes][8 bf16]
    DevBuf stem_w2k;                 // layer 2 again as [tap][input-channel quad][16 output channels][4] for the 4-block f32 MFMA
    // layer 1 with Preprocessor.process folded in, for uint8 patches (vt_stem.h: L1In): [162 weights][6 biases][3 pad values]
    DevBuf stem_w1u;
    std::vector<double> stem_w1_f64, stem_b1_f64;   // layer 1 with BN folded, kept for vt_set_normalization
    float norm_mean[3] = {0.485f, 0.456f, 0.406f}, norm_std[3] = {0.229f, 0.224f, 0.225f};   // lib/test/tracker/data_utils.py:8-9
    DevBuf pos_z, pos_x;             // (len, C)
    DevBuf blocks;                   // depth * BLOCK_STRIDE + 2C (final norm)
    DevBuf blocks3;                  // depth * BLOCK3_STRIDE: the MLP's three-piece bf16 images (vt_blocks.h, BF3)
    DevBuf head;                     // 3 * TOWER_STRIDE
    DevBuf head3;                    // F = 8, fp32 build: the towers' weights as three-piece bf16 images (vt_head3.h)
    DevBuf window;                   // F*F
    // workspace sized for max_batch
    DevBuf act_x, act_z;             // layer-2 activations, NHWC(12)
    DevBuf tokens, feat;
    DevBuf tokens_c;                 // token matrix of the cached-template step: its template rows are written by vt_set_template only
    // small batches (vt_blocks_tile.h): q / K image / V^T image of every tile and the residual stream between the per-block launches
    DevBuf tile_q, tile_k, tile_v, tile_x;
    DevBuf head_m1;                  // F = 16, small batches: conv1 output of the three towers, [frames][3][8][NPIX] float4, zero borders
    int head_m1_frames = 0;
    int tile_frames = 0;             // frames those workspaces are sized for
    int open_loop = 0;               // vt_set_open_loop: vt_track_step leaves states_dev untouched (the step's box is in `record`)
    DevBuf zcache;                   // block-0 q / k / v^T images of the template tiles (vt_set_template)
    DevBuf imsizes;                  // vt_track_step_images: (max_batch,) vt_frame sizes of the step's descriptors, written by its crop for the tail
    DevBuf zstage;                   // vt_set_template_slots: the new slots' cache rows, staged before they are copied into place (allocated on first use)
    DevBuf vlscr;                    // G256 frame-form block kernel (A3): the low pieces of V^T, [B][depth][3][L / 32][64] x 16 B (vt_blocks.h VP2L)
    int tmpl_frames = 0;             // frames whose template rows (tokens + zcache) are cached
    int tmpl_form_batch = 0;         // the form batch vt_set_template ran under (the cache holds THAT form's operands)
    int graphs_captured = 0;         // live graphs captured from this model (vt_graph_destroy takes them off again): they hold the forms of their capture
    std::vector<vt_graph*> graphs;   // those graphs; vt_destroy orphans them, so a graph destroyed after its model touches nothing of it
    DevBuf score, size, offset, pred, hann, conf;
    hipStream_t cap_stream = nullptr;
    hipStream_t side_stream[3] = {nullptr, nullptr, nullptr};   // extra capture streams for graph chains
    hipEvent_t fork_ev = nullptr, join_ev[3] = {nullptr, nullptr, nullptr};
    unsigned long long* dbg_stamps = nullptr;   // VT_DBG_STAMPS=1: per-wave phase stamps of the block kernel
    int form_batch = 0;    // vt_set_form_batch: kernel forms are chosen as for a batch of this size (0: by the batch of each call)
    int plan_r2[2] = {0, 0}, plan_r4[2] = {0, 0};   // band plan for (search, template) crops
};

struct vt_graph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    vt_model* owner = nullptr;      // its capture counts in owner->graphs_captured until vt_graph_destroy (the model must outlive its graphs)
};

namespace {

int check_ready(vt_model* m, int B) {
    if (!m) return fail(VT_ERR_ARG, "null model");
    if (!m->weights_loaded) return fail(VT_ERR_STATE, "vt_load_weights has not been called");
    if (B < 1 || B > m->cfg.max_batch)
        return fail(VT_ERR_STATE, "batch " + std::to_string(B) + " outside [1, max_batch=" + std::to_string(m->cfg.max_batch) + "]");
    return VT_OK;
}

// The batch size the kernel FORMS of a call are chosen by: the call's own, or the model's form batch (vt_set_form_batch) -- a shard
// of a larger group of sequences then runs the forms the whole group would, so its results do not depend on how the group is sharded.
int form_b(const vt_model* m, int B) { return std::max(B, m->form_batch); }

// Band sizes per crop side.  stem_a: r2 layer-2 rows per workgroup (256 output pixels);
// stem_b: r4 token rows per workgroup (LDS <= ~50 KB so three workgroups share a CU).
struct StemPlan { int r2, r4; };
StemPlan stem_plan(int T) {   // VT_STEM_R2_<T> / VT_STEM_R4_<T> override the defaults (tuning aid)
    StemPlan p{0, 0};
    switch (T) {
        case 64: p = {16, 4}; break;    // layer-2 map 16x16, tokens 4x4: one band each
        case 128: p = {8, 4}; break;    // 32x32 -> 4 bands; tokens 8x8 -> 2 bands
        case 256: p = {4, 2}; break;    // 64x64 -> 16 bands; tokens 16x16 -> 8 bands
    }
    const std::string t = std::to_string(T);
    p.r2 = env_int(("VT_STEM_R2_" + t).c_str(), p.r2);
    p.r4 = env_int(("VT_STEM_R4_" + t).c_str(), p.r4);
    return p;
}

// floats of V^T low-piece scratch per frame (vt_blocks.h VP2L): depth x NC feature tiles x L / 32 chunk pairs x 64 lanes x 16 B
size_t vlscr_floats_per_frame(const vt_model* m) { return (size_t)m->cfg.depth * vtb::NC * (m->L / 32) * 64 * 4; }

#ifdef VT_F16
// a conv weight image in place: every 16-byte slot's float4 becomes h4 in its first 8 bytes (vt_conv.h load_weights)
__global__ void opnd_inplace_kernel(float* __restrict__ img, size_t n4) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n4) {
        const opnd v = to_opnd(ld4(img + 4 * i));
        *reinterpret_cast<opnd*>(img + 4 * i) = v;
    }
}
int opnd_inplace(float* img, size_t nfloats) {
    hipLaunchKernelGGL(opnd_inplace_kernel, dim3((unsigned)((nfloats / 4 + 255) / 256)), dim3(256), 0, nullptr, img, nfloats / 4);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return VT_OK;
}
// float4 -> h4 (the MFMA operand conversion of vt_common.h), n4 quads
__global__ void f32_to_opnd_kernel(const float* __restrict__ src, _Float16* __restrict__ dst, size_t n4) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n4) reinterpret_cast<opnd*>(dst)[i] = to_opnd(ld4(src + 4 * i));
}
#endif

}  // namespace

#include "vt_weights.h"

namespace {

// ---------------------------------------------------------------------------------------- shape-generic path (vt_generic.h)
inline unsigned gen_grid(size_t n) { return (unsigned)((n + 255) / 256); }

int gen_stem(vt_model* m, const float* z, const float* x, int B, hipStream_t st, float* tokens, int zmode, bool xu8 = false) {
    for (int side = 0; side < 2; ++side) {       // 0: template rows, 1: search rows
        const float* img = side == 0 ? z : x;
        if ((side == 0 && zmode == 1) || (side == 1 && zmode == 2) || !img) continue;
        const int T = side == 0 ? m->cfg.template_size : m->cfg.search_size;
        const float* in = img;
        int S = T;
        const int C = m->gd.C, chans[5] = {3, C / 8, C / 4, C / 2, C};      // b16 (vit_dist.py:36-54)
        for (int i = 0; i < 4; ++i) {
            const int cin = chans[i], cout = chans[i + 1], So = S / 2;
            float* out = (i & 1) ? m->g_b.p : m->g_a.p;
            const size_t total = (size_t)B * cout * So * So;
            if (i == 0 && side == 1 && xu8) {      // the search crop arrives as sample_target's uint8 patch: Preprocessor.process per tap, same weights
                hipLaunchKernelGGL(vtg::stem_conv_u8_kernel, dim3(gen_grid(total)), dim3(256), 0, st, reinterpret_cast<const unsigned char*>(img), m->g_stem_w[0].p,
                                   m->g_stem_b[0].p, B, cout, S, m->norm_mean[0], m->norm_mean[1], m->norm_mean[2], m->norm_std[0], m->norm_std[1],
                                   m->norm_std[2], out);
                in = out;
                S = So;
                continue;
            }
            hipLaunchKernelGGL(vtg::stem_conv_kernel, dim3(gen_grid(total)), dim3(256), 0, st, in, m->g_stem_w[i].p, m->g_stem_b[i].p, B, cin, cout, S,
                               i < 3 ? out : nullptr, i < 3 ? nullptr : tokens, side == 0 ? m->pos_z.p : m->pos_x.p, m->L, side == 0 ? 0 : m->len_z);
            in = out;
            S = So;
        }
    }
    HIP_TRY(hipGetLastError());
    return VT_OK;
}

int gen_blocks(vt_model* m, const float* tokens, int B, int nblocks, hipStream_t st, float* feat, float* resid) {
    if (nblocks < 0 || nblocks > m->cfg.depth) nblocks = m->cfg.depth;
    const size_t rows = (size_t)B * m->L;
    // the residual stream is updated in place in a buffer of its own: the caller's tokens -- and the cached template rows of
    // vt_set_template's token matrix -- stay untouched
    float* x = m->g_x.p;
    const vtg::Dims d = m->gd;
    const int C = d.C, HID = d.hid();
    HIP_TRY(hipMemcpyAsync(x, tokens, rows * C * sizeof(float), hipMemcpyDeviceToDevice, st));
    for (int i = 0; i < nblocks; ++i) {
        const float* P = m->g_blocks.p + (size_t)i * d.block_stride();
        hipLaunchKernelGGL(vtg::ln_linear_kernel<0>, dim3(gen_grid(rows * 3 * C)), dim3(256), 0, st, x, P + d.o_wqkv(), P + d.o_bqkv(), rows, C, 3 * C, m->g_qkv.p);
        const unsigned ag = gen_grid(rows * d.heads);
        switch (d.hd()) {       // head_dim as a template value where it is a common one (registers), else the run-time form
            case 16: hipLaunchKernelGGL(vtg::attn_kernel<16>, dim3(ag), dim3(256), 0, st, m->g_qkv.p, B, m->L, C, d.heads, m->g_ao.p); break;
            case 32: hipLaunchKernelGGL(vtg::attn_kernel<32>, dim3(ag), dim3(256), 0, st, m->g_qkv.p, B, m->L, C, d.heads, m->g_ao.p); break;
            case 48: hipLaunchKernelGGL(vtg::attn_kernel<48>, dim3(ag), dim3(256), 0, st, m->g_qkv.p, B, m->L, C, d.heads, m->g_ao.p); break;
            case 64: hipLaunchKernelGGL(vtg::attn_kernel<64>, dim3(ag), dim3(256), 0, st, m->g_qkv.p, B, m->L, C, d.heads, m->g_ao.p); break;
            default: hipLaunchKernelGGL(vtg::attn_kernel<0>, dim3(ag), dim3(256), 0, st, m->g_qkv.p, B, m->L, C, d.heads, m->g_ao.p); break;
        }
        hipLaunchKernelGGL(vtg::linear_resid_kernel, dim3(gen_grid(rows * C)), dim3(256), 0, st, m->g_ao.p, P + d.o_wproj(), P + d.o_bproj(), rows, C, C, x);
        hipLaunchKernelGGL(vtg::ln_linear_kernel<1>, dim3(gen_grid(rows * HID)), dim3(256), 0, st, x, P + d.o_w1(), P + d.o_b1(), rows, C, HID, m->g_hid.p);
        hipLaunchKernelGGL(vtg::linear_resid_kernel, dim3(gen_grid(rows * C)), dim3(256), 0, st, m->g_hid.p, P + d.o_w2(), P + d.o_b2(), rows, C, HID, x);
    }
    if (resid) HIP_TRY(hipMemcpyAsync(resid, x, rows * C * sizeof(float), hipMemcpyDeviceToDevice, st));
    const float* N = m->g_blocks.p + (size_t)m->cfg.depth * d.block_stride();
    hipLaunchKernelGGL(vtg::final_norm_kernel, dim3(gen_grid((size_t)B * m->len_x * C)), dim3(256), 0, st, x, N, N + C, B, m->L, m->len_z, C, feat);
    HIP_TRY(hipGetLastError());
    return VT_OK;
}

int gen_head(vt_model* m, const float* feat, int B, hipStream_t st, float* score, float* size, float* offset) {
    const int F = m->F;
    const vtg::Dims d = m->gd;
    const size_t npx = (size_t)B * F * F;
    const float* in = feat;
    size_t in_stride = 0;
    for (int i = 0; i < 4; ++i) {
        float* out = (i & 1) ? m->g_b.p : m->g_a.p;
        hipLaunchKernelGGL(vtg::head_conv_kernel, dim3(gen_grid(3 * npx * d.hch(i + 1))), dim3(256), 0, st, in, in_stride, m->g_head.p, d.tower_stride(),
                           d.ho_w(i), d.ho_b(i), B, F, d.hch(i), d.hch(i + 1), out);
        in = out;
        in_stride = npx * d.hch(i + 1);
    }
    hipLaunchKernelGGL(vtg::head_out_kernel, dim3(gen_grid(npx)), dim3(256), 0, st, in, m->g_head.p, d.tower_stride(), d.ho_w5(), d.ho_b5(), d.hch(4), B, F,
                       score, size, offset);
    HIP_TRY(hipGetLastError());
    return VT_OK;
}

// Graph chains: a chain may start late (VT_CHAIN_DELAY_US x chain index), so that identical chains do not run in lock step
__global__ void chain_delay_kernel(unsigned long long ticks) {      // 100 MHz ticks
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}

// ------------------------------------------------------------------------------------ self test
__global__ void mfma_selftest_kernel(const float* A, const float* Bm, float* D) {
    // A (16x16 k-chunk as operand image source: A[i][k]), B[k][j]; D[i][j] = sum_k A[i][k] B[k][j]
    const int lane = threadIdx.x, rc = lane & 15, q = lane >> 4;
    f4 a, b;
    for (int r = 0; r < 4; ++r) {
        a[r] = A[rc * 16 + 4 * q + r];
        b[r] = Bm[(4 * q + r) * 16 + rc];
    }
    f4 acc = mfma4(a, b, splat4(0.f));
    for (int r = 0; r < 4; ++r) D[(4 * q + r) * 16 + rc] = acc[r];
    // permlane-swap reductions over the 4 lanes sharing (lane & 15): sum must be 15 (rc + 1), max 8 (rc + 1)
    const float v = (float)((1 << q) * (rc + 1));
    D[256 + lane] = quad_sum(v);
    D[320 + lane] = quad_max(v);
}

// Clock / MFMA-rate probe: every wave runs `iters` rounds of 8 independent v_mfma_f32_16x16x4_f32
// and stamps the shader clock (s_memtime) and the constant 100 MHz clock (s_memrealtime).
__global__ __launch_bounds__(256) void probe_kernel(const float* __restrict__ src, int iters,
                                                    unsigned long long* __restrict__ stamps, float* __restrict__ sink) {
    f4 acc[8];
    const float a0 = src[threadIdx.x], b0 = src[256 + threadIdx.x];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = splat4(0.001f * j);
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[j], 0, 0, 0);
    }
    f4 sum = splat4(0.f);
#pragma unroll
    for (int j = 0; j < 8; ++j) sum = sum + acc[j];
    sink[(size_t)blockIdx.x * 256 + threadIdx.x] = sum.x + sum.y + sum.z + sum.w;   // data dependence on every MFMA
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if ((threadIdx.x & 63) == 0) {
        const size_t k = ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 2;
        stamps[k] = t1 - t0;
        stamps[k + 1] = r1 - r0;
    }
}

// ------------------------------------------------------------------------------------------ forms
// THE place where kernel forms are chosen.  Every instantiation of a kernel family shares one signature, so a family is a
// table of plain function pointers: one entry per instantiation with the mode values it serves, its workgroup size and its dynamic LDS.
// A stage's selector (select_stem / select_blocks / select_head) maps the model's switches and geometry, the form batch and the call's
// mode to entries; the launch uses what it returns, and vt_create opts every entry into its dynamic LDS (for_each_lds_form) -- an
// instantiation and its LDS size are named once, here.
template <class K> struct FormEntry {
    std::array<int, 4> key;
    K k;
    unsigned block;      // threads per workgroup
    size_t lds;          // dynamic LDS bytes
};
template <class K> constexpr FormEntry<K> form(std::array<int, 4> key, K k, unsigned block, size_t lds) { return {key, k, block, lds}; }
template <class Tab> const typename Tab::value_type* find_form(const Tab& tab, std::array<int, 4> key) {
    for (const auto& e : tab)
        if (e.key == key) return &e;
    return nullptr;
}

#ifndef VT_F16
// key: search size, zmode, uint8 patch
const std::array STEM_STREAM = {
    form({256, 0, 0}, &vts::stem_stream_kernel<256, 128, 0>, 1024, vts::StreamGeo<256, 128>::LDS_BYTES),
    form({256, 1, 0}, &vts::stem_stream_kernel<256, 128, 1>, 1024, vts::StreamGeo<256, 128>::LDS_BYTES),
    form({256, 2, 0}, &vts::stem_stream_kernel<256, 128, 2>, 1024, vts::StreamGeo<256, 128>::LDS_BYTES),
    form({256, 1, 1}, &vts::stem_stream_kernel<256, 128, 1, true>, 1024, vts::StreamGeo<256, 128>::LDS_BYTES),
    form({128, 0, 0}, &vts::stem_stream_kernel<128, 64, 0>, 1024, vts::StreamGeo<128, 64>::LDS_BYTES),
    form({128, 1, 0}, &vts::stem_stream_kernel<128, 64, 1>, 1024, vts::StreamGeo<128, 64>::LDS_BYTES),
    form({128, 2, 0}, &vts::stem_stream_kernel<128, 64, 2>, 1024, vts::StreamGeo<128, 64>::LDS_BYTES),
    form({128, 1, 1}, &vts::stem_stream_kernel<128, 64, 1, true>, 1024, vts::StreamGeo<128, 64>::LDS_BYTES),
};
#endif
// key: zmode, diagnostic build, layer 3 as BF3 products (VT_STEM_BF3; 0: fp32 MFMAs, the all-fp32-MFMA step bench.py reports beside the
// default), uint8 patch
const std::array STEM_FUSED = {
    form({0, 0, 1, 0}, &vts::stem_fused_kernel<0, false>, 1024, (size_t)vts::FusedGeo::LDS_BYTES_P),
    form({1, 0, 1, 0}, &vts::stem_fused_kernel<1, false>, 1024, (size_t)vts::FusedGeo::LDS_BYTES_P),
    form({2, 0, 1, 0}, &vts::stem_fused_kernel<2, false>, 1024, (size_t)vts::FusedGeo::LDS_BYTES_P),
    form({0, 1, 1, 0}, &vts::stem_fused_kernel<0, true>, 1024, (size_t)vts::FusedGeo::LDS_BYTES_P),
    form({0, 0, 0, 0}, &vts::stem_fused_kernel<0, false, false>, 1024, (size_t)vts::FusedGeo::LDS_BYTES_P),
    form({1, 0, 0, 0}, &vts::stem_fused_kernel<1, false, false>, 1024, (size_t)vts::FusedGeo::LDS_BYTES_P),
    form({2, 0, 0, 0}, &vts::stem_fused_kernel<2, false, false>, 1024, (size_t)vts::FusedGeo::LDS_BYTES_P),
    form({1, 0, 1, 1}, &vts::stem_fused_kernel<1, false, true, true>, 1024, (size_t)vts::FusedGeo::LDS_BYTES_P),
    form({1, 0, 0, 1}, &vts::stem_fused_kernel<1, false, false, true>, 1024, (size_t)vts::FusedGeo::LDS_BYTES_P),
};
// key: zmode, diagnostic build, uint8 patch
const std::array STEM_PIPE = {
    form({0, 0, 0}, &vts::stem_pipe_kernel<256, 128, 0, false>, 1024, vts::PipeGeo<256, 128>::LDS_BYTES),
    form({1, 0, 0}, &vts::stem_pipe_kernel<256, 128, 1, false>, 1024, vts::PipeGeo<256, 128>::LDS_BYTES),
    form({2, 0, 0}, &vts::stem_pipe_kernel<256, 128, 2, false>, 1024, vts::PipeGeo<256, 128>::LDS_BYTES),
    form({0, 1, 0}, &vts::stem_pipe_kernel<256, 128, 0, true>, 1024, vts::PipeGeo<256, 128>::LDS_BYTES),
    form({1, 0, 1}, &vts::stem_pipe_kernel<256, 128, 1, false, true>, 1024, vts::PipeGeo<256, 128>::LDS_BYTES),
};
// key: uint8 patch (stem_a) / diagnostic build (stem_b); their LDS follows the band plan (select_stem)
const std::array STEM_A = {form({0}, &vts::stem_a_kernel<false>, 256, 0), form({1}, &vts::stem_a_kernel<true>, 256, 0)};
const std::array STEM_B = {form({0}, &vts::stem_b_kernel<false>, 256, 0), form({1}, &vts::stem_b_kernel<true>, 256, 0)};

// The frame form of the blocks: the template arguments as values; the LDS depends on the model's depth (blocks_lds_bytes)
struct BlocksKey {
    int NT, NW, TPW;
    bool WLDS, BAL, ZC, BF3, A3;
    bool operator==(const BlocksKey& o) const {
        return NT == o.NT && NW == o.NW && TPW == o.TPW && WLDS == o.WLDS && BAL == o.BAL && ZC == o.ZC && BF3 == o.BF3 && A3 == o.A3;
    }
    size_t lds(int depth) const { return blocks_lds_bytes(NT, WLDS, BAL, depth, BF3, A3); }
};
template <class K> struct BlocksEntry { BlocksKey key; K k; };
template <int NT, int NW, int TPW, bool WLDS, bool BAL = false, bool ZC = false, bool BF3 = false, bool A3 = false> constexpr auto blocks_form() {
    constexpr auto k = &vtb::blocks_kernel<NT, NW, TPW, WLDS, BAL, ZC, BF3, A3>;
    return BlocksEntry<decltype(k)>{{NT, NW, TPW, WLDS, BAL, ZC, BF3, A3}, k};
}
const std::array BLOCKS = {
    blocks_form<5, 5, 1, true>(), blocks_form<5, 5, 1, false>(),                                   // G128, one wave per tile (VT_BLOCKS_BAL=0)
    blocks_form<5, 8, 1, true, true>(), blocks_form<5, 8, 1, true, true, true>(),                  // G128, balanced; fp32 MFMAs
    // G256.  8 waves: waves s and s+4 share SIMD s with 3 + 2 tiles, so each SIMD has two instruction streams
    blocks_form<20, 4, 5, false>(), blocks_form<20, 8, 3, false>(), blocks_form<20, 8, 3, false, false, true>(),
#ifndef VT_F16
    blocks_form<5, 8, 1, true, true, false, true>(), blocks_form<5, 8, 1, true, true, true, true>(),                  // VT_BLOCKS_BF3=1
    blocks_form<5, 8, 1, true, true, false, true, true>(), blocks_form<5, 8, 1, true, true, true, true, true>(),      // 2 (default)
    blocks_form<20, 8, 3, false, false, false, true>(), blocks_form<20, 8, 3, false, false, true, true>(),
    blocks_form<20, 8, 3, false, false, false, true, true>(), blocks_form<20, 8, 3, false, false, true, true, true>(),
#endif
};

// The head in ONE kernel per frame, decode included (F = 8: towers side by side; F = 16: the three towers in turn).  key: F, diagnostic build
const std::array HEAD_WHOLE = {
    form({8, 0}, &vth::head_fused_kernel<8, false>, 768, (size_t)vth::FusedHeadGeo<8>::LDS_BYTES),
    form({8, 1}, &vth::head_fused_kernel<8, true>, 768, (size_t)vth::FusedHeadGeo<8>::LDS_BYTES),
    form({16, 0}, &vth::head_seq_kernel<16, 8, false>, 512, (size_t)vth::SeqHeadGeo<16>::LDS_BYTES),
    form({16, 1}, &vth::head_seq_kernel<16, 8, true>, 512, (size_t)vth::SeqHeadGeo<16>::LDS_BYTES),
};
// One workgroup per (frame, tower); decode_kernel follows.  key: F, diagnostic build, input = conv1's output (after head_conv1_kernel).
// F = 16: 129 KB of LDS per tower = one workgroup per CU: 8 waves give every SIMD two instruction streams
const std::array HEAD_TOWERS = {
    form({8, 0, 0}, &vth::head_towers_kernel<8, 4, false>, 256, (size_t)vth::Geo<8>::LDS_BYTES),
    form({8, 1, 0}, &vth::head_towers_kernel<8, 4, true>, 256, (size_t)vth::Geo<8>::LDS_BYTES),
    form({16, 0, 0}, &vth::head_towers_kernel<16, 8, false>, 512, (size_t)vth::Geo<16>::LDS_BYTES),
    form({16, 1, 0}, &vth::head_towers_kernel<16, 8, true>, 512, (size_t)vth::Geo<16>::LDS_BYTES),
    form({16, 0, 1}, &vth::head_towers_kernel<16, 8, false, true>, 512, (size_t)vth::Geo<16>::LDS_BYTES),
};
#ifndef VT_F16
// the three-piece bf16 towers (vt_head3.h).  F = 8: whole head / per tower; F = 16: head_seq3 (conv1 as BF3 products; key: phase stamps)
const std::array HEAD_FUSED3 = {form({8}, &vth3::head_fused3_kernel, 768, (size_t)vth3::FUSED3_LDS_BYTES)};
const std::array HEAD_TOWERS3 = {form({8}, &vth3::head_towers3_kernel, 256, (size_t)vth3::TOWERS3_LDS_BYTES)};
const std::array HEAD_SEQ3 = {
    form({0}, &vth3::head_seq3_kernel<8, VT_SEQ3_MAXP, false>, 512, (size_t)vth3::SEQ3_LDS_BYTES),
    form({1}, &vth3::head_seq3_kernel<8, VT_SEQ3_MAXP, true>, 512, (size_t)vth3::SEQ3_LDS_BYTES),
};
#endif

// f(kernel, bytes) for every form of the model that is launched with dynamic LDS: > 64 KiB needs an explicit opt-in, which vt_create
// makes once (not at the launch: a launch may be under stream capture).  Block kernels: the model's own token count, and the BF3 levels
// its depth leaves room for (read_switches).
template <class F> void for_each_lds_form(const vt_model* m, F&& f) {
    auto all = [&](const auto& tab) { for (const auto& e : tab) f(reinterpret_cast<const void*>(e.k), e.lds); };
    all(STEM_FUSED); all(STEM_PIPE); all(HEAD_WHOLE); all(HEAD_TOWERS);
#ifndef VT_F16
    all(STEM_STREAM); all(HEAD_FUSED3); all(HEAD_TOWERS3); all(HEAD_SEQ3);
#endif
    for (const auto& e : BLOCKS) {
        const int bf3 = e.key.NT == 5 ? m->sw.blocks_bf3 : m->sw.blocks_bf3_g256;
        if (e.key.NT == m->L / 16 && (e.key.A3 ? bf3 >= 2 : e.key.BF3 ? bf3 >= 1 : true)) f(reinterpret_cast<const void*>(e.k), e.key.lds(m->cfg.depth));
    }
}

// ---- stem
// zmode 0: both crops; 1: search crop only (template token rows already in `tokens`); 2: template crop only
// xu8: x is a uint8 (B, Tx, Tx, 3) patch (vt_crop_u8) and layer 1 runs on the folded weights w1u; zmode 1 only
struct StemForm {
    // at most one of the one-workgroup-per-frame kernels ...
#ifndef VT_F16
    const decltype(STEM_STREAM)::value_type* stream = nullptr;     // all four layers: nothing but token rows leaves the CU
#endif
    const decltype(STEM_FUSED)::value_type* fused = nullptr;       // G128, the same
    const decltype(STEM_PIPE)::value_type* pipe = nullptr;         // G256, layers 1 + 2 (two wave groups half a period apart); stem_b follows
    // ... else the banded form: stem_a (or stem_a2: band k of both crops in one workgroup), then stem_b
    const decltype(STEM_A)::value_type* a = nullptr;
    bool a2 = false;
    const decltype(STEM_B)::value_type* b = nullptr;
    StemPlan px{}, pz{};       // rows per band: (search, template) crop; pz.r2 is the fused form's when a2
    size_t lds_a = 0, lds_b = 0;
};

int select_stem(const vt_model* m, int Bf, int zmode, bool xu8, StemForm* f) {
    const Switches& s = m->sw;
    const bool diag_a = s.skip_stem_a != 0 || m->dbg_stamps != nullptr, diag = diag_a || s.skip_stem_b != 0;
    // every form of the tuned geometries reads uint8 patches (stem_fused, stem_stream, stem_pipe, stem_a); the diagnostic builds do not
    if (xu8 && (zmode != 1 || diag)) return fail(VT_ERR_STATE, "this stem form has no uint8-patch variant");
    const int Tx = m->cfg.search_size, Tz = m->cfg.template_size;
    StemPlan px{m->plan_r2[0], m->plan_r4[0]};
    StemPlan pz{m->plan_r2[1], m->plan_r4[1]};
    // small batches of the 128-px search crop: stem_b in bands of 2 token rows (4 workgroups per crop instead of 2) shortens the
    // latency chain of a band (B=1 step 63.5 -> 59.9 us); at large batches the halo rows it recomputes cost more than that
    if (Tx == 128 && Bf <= 80 && px.r4 == 4 && !s.r4_128_forced) px.r4 = 2;
    for (const auto& pr : {std::make_pair(Tx, px), std::make_pair(Tz, pz)}) {
        const int T = pr.first, r2 = pr.second.r2, r4 = pr.second.r4;
        const int nt4 = r4 > 0 ? (r4 * (T / 16) + 15) / 16 : 0;
        if (r2 < 1 || r4 < 1 || (T / 4) % r2 || (T / 16) % r4 || (r2 * (T / 4)) % 256 || !(nt4 == 1 || nt4 == 2 || nt4 == 4) ||
            (r4 * (T / 16)) % 16 || (((2 * r4 + 1) * (T / 8)) % 16 && ((2 * r4) * (T / 8)) % 16) ||
            3 * vts::stem_b_npix2(T / 4, r4) < 4 * nt4 * 3 * 64 ||
            (T / 4) > 256 || (4 * r4 + 3) > 5 * (256 / (T / 4)))     // stem_b stages <= 5 layer-2 rows per thread and plane
            return fail(VT_ERR_ARG, "unsupported stem band plan for crop side " + std::to_string(T));
    }
    const bool g256 = Tx == 256 && Tz == 128;
#ifndef VT_F16
    const bool g128 = Tx == 128 && Tz == 64;
    if ((s.stem_stream < 0 ? (g256 && Bf > 176) : s.stem_stream != 0) && !diag && (g256 || g128)) {
        f->stream = find_form(STEM_STREAM, {Tx, zmode, xu8});
        return f->stream ? VT_OK : fail(VT_ERR_STATE, "no stem_stream form for this mode");
    }
#endif
    if ((s.stem_fused < 0 ? Bf > 80 : s.stem_fused != 0) && Tx == vts::FusedGeo::TX && Tz == vts::FusedGeo::TZ) {
        if (diag_a && zmode != 0) return fail(VT_ERR_STATE, "the diagnostic stem build has no template-cache form");
        f->fused = find_form(STEM_FUSED, {zmode, diag_a, diag_a || s.stem_bf3 != 0, xu8});     // (the diagnostic build has the default layer 3)
        return f->fused ? VT_OK : fail(VT_ERR_STATE, "no stem_fused form for this mode");
    }
    if ((s.stem_pipe < 0 ? Bf > 176 : s.stem_pipe != 0) && g256) {
        if (diag_a && zmode != 0) return fail(VT_ERR_STATE, "the diagnostic stem build has no template-cache form");
        if (!(f->pipe = find_form(STEM_PIPE, {zmode, diag_a, xu8}))) return fail(VT_ERR_STATE, "no stem_pipe form for this mode");
    } else {
        // stem_a2: band k of both crops in one workgroup, when the template band then has exactly one layer-2 tile per wave and the
        // workgroup count fills whole rounds of 4 per CU better than the split form
        const int bands_x = (Tx / 4) / px.r2, r2z_f = (Tz / 4) / bands_x;
        f->a2 = zmode == 0 && s.stem_fuse && r2z_f >= 1 && r2z_f * bands_x == Tz / 4 && r2z_f * (Tz / 4) == 64;
        if (f->a2) {
            pz.r2 = r2z_f;
            f->lds_a = sizeof(float) * (vts::stem_a_lds_floats(Tx, px.r2) + vts::stem_a_lds_floats(Tz, pz.r2));
        } else {
            f->a = find_form(STEM_A, {xu8});
            f->lds_a = sizeof(float) * std::max(vts::stem_a_lds_floats(Tx, px.r2), vts::stem_a_lds_floats(Tz, pz.r2));
        }
    }
    f->b = find_form(STEM_B, {s.skip_stem_b != 0});
    f->lds_b = std::max(vts::stem_b_lds_bytes(Tx / 4, px.r4), vts::stem_b_lds_bytes(Tz / 4, pz.r4));
    f->px = px;
    f->pz = pz;
    return VT_OK;
}

// Does the stem form a batch of B (under the model's form batch) selects read uint8 patches?
bool stem_takes_u8(const vt_model* m, int B) {
    if (m->vb) return true;          // vitb.hip stem_rows: vbm::patchify_u8_kernel + the normalisation-folded patch weights, at every batch
    if (m->generic) return true;     // vt_generic.h: stem_conv_u8_kernel (the reference's own normalisation per tap)
    StemForm f;
    return m->stem_w1u.p != nullptr && select_stem(m, form_b(m, B), 1, true, &f) == VT_OK;
}

int run_stem(vt_model* m, const float* z, const float* x, int B, hipStream_t st, float* tokens, size_t f0 = 0, int zmode = 0, bool xu8 = false) {
    // f0: first frame of this slice in the model workspace (z, x, tokens already point at the slice)
    if (m->generic) {
        if (xu8 && zmode != 1) return fail(VT_ERR_STATE, "this stem form has no uint8-patch variant");
        return gen_stem(m, z, x, B, st, tokens, zmode, xu8);
    }
    StemForm f;
    if (int rc = select_stem(m, form_b(m, B), zmode, xu8, &f)) return rc;
    const float* const w1 = xu8 ? m->stem_w1u.p : m->stem_w[0].p;
    const float* const b1 = xu8 ? m->stem_w1u.p + vts::W1U_BIAS : m->stem_b[0].p;
    const int Tx = m->cfg.search_size, Tz = m->cfg.template_size;
    float* const act_x = m->act_x.p + f0 * (size_t)(Tx / 4) * (Tx / 4) * 12;
    float* const act_z = m->act_z.p + f0 * (size_t)(Tz / 4) * (Tz / 4) * 12;
    const int skip_a = m->sw.skip_stem_a;
#ifndef VT_F16
    if (f.stream) {
        hipLaunchKernelGGL(f.stream->k, dim3(B), dim3(f.stream->block), f.stream->lds, st, z, x, w1, b1, m->stem_b[1].p, m->stem_w[2].p, m->stem_b[2].p,
                           m->stem_w[3].p, m->stem_b[3].p, m->pos_z.p, m->pos_x.p, tokens, m->L, m->len_z, m->stem_w2k.p);
        HIP_TRY(hipGetLastError());
        return VT_OK;
    }
#endif
    if (f.fused) {
        hipLaunchKernelGGL(f.fused->k, dim3(B), dim3(f.fused->block), f.fused->lds, st, z, x, w1, b1, m->stem_w[1].p, m->stem_b[1].p, m->stem_w[2].p,
                           m->stem_b[2].p, m->stem_w[3].p, m->stem_b[3].p, m->pos_z.p, m->pos_x.p, tokens, m->L, m->len_z, skip_a, m->dbg_stamps,
                           m->stem_w2k.p, m->stem_w3b.p, m->stem_w4b.p);
        HIP_TRY(hipGetLastError());
        return VT_OK;
    }
    // zmode (template cache): a crop that is not wanted gets zero bands -- stem_a / stem_b index their workgroups by
    // (frame, band of x | band of z), so its workgroups simply do not exist
    vts::CropA ax{x, act_x, Tx, f.px.r2, zmode == 2 ? 0 : (Tx / 4) / f.px.r2}, az{z, act_z, Tz, f.pz.r2, zmode == 1 ? 0 : (Tz / 4) / f.pz.r2};
    if (f.pipe)
        hipLaunchKernelGGL(f.pipe->k, dim3(B), dim3(f.pipe->block), f.pipe->lds, st, z, x, w1, b1, m->stem_w[1].p, m->stem_b[1].p, act_z, act_x, skip_a,
                           m->dbg_stamps, m->stem_w2k.p);
    else if (f.a2)
        hipLaunchKernelGGL(vts::stem_a2_kernel, dim3(B * ax.bands), dim3(256), f.lds_a, st, ax, az, m->stem_w[0].p, m->stem_b[0].p, m->stem_w[1].p,
                           m->stem_b[1].p, skip_a);
    else
        hipLaunchKernelGGL(f.a->k, dim3(B * (ax.bands + az.bands)), dim3(f.a->block), f.lds_a, st, ax, az, w1, b1, m->stem_w[1].p, m->stem_b[1].p, skip_a);
    HIP_TRY(hipGetLastError());
    vts::CropB bx{act_x, m->pos_x.p, Tx / 4, f.px.r4, zmode == 2 ? 0 : (Tx / 16) / f.px.r4, m->len_z};
    vts::CropB bz{act_z, m->pos_z.p, Tz / 4, f.pz.r4, zmode == 1 ? 0 : (Tz / 16) / f.pz.r4, 0};
    hipLaunchKernelGGL(f.b->k, dim3(B * (bx.bands + bz.bands)), dim3(f.b->block), f.lds_b, st, bx, bz, m->stem_w[2].p, m->stem_b[2].p, m->stem_w[3].p,
                       m->stem_b[3].p, tokens, m->L, m->sw.skip_stem_b);
    HIP_TRY(hipGetLastError());
    return VT_OK;
}

// ---- blocks
struct BlocksForm {
    int tile_nt = 0;                                           // small batches: one wave per (tile, frame), two launches per block (vt_blocks_tile.h)
    const decltype(BLOCKS)::value_type* frame = nullptr;       // else one workgroup per frame
};

// zc: template cache mode of block 0 (0 off, 1 store, 2 load); f0: first frame of this slice in the model workspace
int select_blocks(const vt_model* m, int Bf, int B, int nblocks, int zc, size_t f0, BlocksForm* f) {
    const Switches& s = m->sw;
    // Kernel form by batch size: with few frames a workgroup per frame leaves most of the chip idle (a frame's latency is one
    // CU's worth of MFMA issue); one wave per tile spreads frames x tiles over the SIMDs instead.
    const int NT = m->L / 16;
    if (NT != 5 && NT != 20) return fail(VT_ERR_ARG, "unsupported token count " + std::to_string(m->L));
    const bool diag = s.dbg_skip_tile != -1 || m->dbg_stamps != nullptr;
    // measured (tools/small_batch_sweep.py, SWEEP_TILE=1; us per step, frame form -> tile form): G256 B=1 281 -> 86, B=32 300 -> 136,
    // B=64 314 -> 183, B=128 371 -> 315; G128 B=1 78 -> 59, B=16 79 -> 62, B=64 84 -> 83, B=80 88 -> 86, B=96 95 -> 95
    const bool want_tile = s.blocks_tile < 0 ? (NT == 20 ? Bf <= 128 : Bf <= 80) : s.blocks_tile != 0;
    if (want_tile && !diag && nblocks >= 1 && f0 + (size_t)B <= (size_t)m->tile_frames) {
        f->tile_nt = NT;
        return VT_OK;
    }
    if (zc != 0 && !s.blocks_bal) return fail(VT_ERR_STATE, "the template cache needs the default block kernel (VT_BLOCKS_BAL = 1)");
    const int bf3 = VT_IS_F16 ? 0 : (NT == 5 ? s.blocks_bf3 : s.blocks_bf3_g256);
    BlocksKey want;
    if (s.blocks_bal) want = NT == 5 ? BlocksKey{5, 8, 1, true, true, zc != 0, bf3 >= 1, bf3 >= 2} : BlocksKey{20, 8, 3, false, false, zc != 0, bf3 >= 1, bf3 >= 2};
    else want = NT == 5 ? BlocksKey{5, 5, 1, s.blocks_wlds != 0, false, false, false, false} : BlocksKey{20, 4, 5, false, false, false, false, false};
    for (const auto& e : BLOCKS)
        if (e.key == want) f->frame = &e;
    return f->frame ? VT_OK : fail(VT_ERR_STATE, "no block kernel of this form");
}

// two workspace sets: a block reads q / K / V^T from one while its workgroups write the next block's into the other.
// f0 = first frame of this slice in the model workspace: the chains of a multi-chain graph (vt_graph_capture_steps) run
// concurrently on different slices, so each works in its own part of every workspace.
template <int NT>
int launch_blocks_tile(vt_model* m, hipStream_t st, const float* tokens, int B, int nblocks, float* feat, float* resid, int zc, size_t f0) {
    const size_t set = (size_t)m->tile_frames * m->L * 48 / 4;                  // float4 per set
    const size_t sl = f0 * m->L * 48 / 4;                                       // float4 offset of the slice inside a set
    f4* const qb = reinterpret_cast<f4*>(m->tile_q.p) + sl;
    f4* const kb = reinterpret_cast<f4*>(m->tile_k.p) + sl;
    f4* const vb = reinterpret_cast<f4*>(m->tile_v.p) + sl;
    float* const tile_x = m->tile_x.p + f0 * m->L * 48;
    const float* const normP = m->blocks.p + (size_t)m->cfg.depth * vtb::BLOCK_STRIDE;      // norm.weight, norm.bias
    hipLaunchKernelGGL((vtb::tile_qkv_kernel<NT>), dim3(NT, B), dim3(64), 0, st, tokens, m->blocks.p, qb, kb, vb, m->zcache.p, zc, m->len_z);
    for (int blk = 0; blk < nblocks; ++blk) {
        const float* P = m->blocks.p + (size_t)blk * vtb::BLOCK_STRIDE;
        const float* xin = blk == 0 ? tokens : tile_x;
        const bool last = blk == nblocks - 1;
        const int skip_z = (blk == m->cfg.depth - 1 && resid == nullptr) ? 1 : 0;
        const size_t cur = (size_t)(blk & 1) * set, nxt = (size_t)((blk & 1) ^ 1) * set;
        hipLaunchKernelGGL((vtb::tile_attn_mlp_kernel<NT>), dim3(NT, B), dim3(256), 0, st, xin, tile_x, P, qb + cur, kb + cur, vb + cur,
                           last ? normP : nullptr, feat, last ? resid : nullptr, m->len_z, skip_z,
                           last ? nullptr : P + vtb::BLOCK_STRIDE, qb + nxt, kb + nxt, vb + nxt);
    }
    HIP_TRY(hipGetLastError());
    return VT_OK;
}

int run_blocks(vt_model* m, const float* tokens, int B, int nblocks, hipStream_t st, float* feat, float* resid, int zc = 0, size_t f0 = 0) {
    if (zc != 0 && f0 != 0) return fail(VT_ERR_STATE, "the template cache is not sliced");
    if (m->generic) return zc == 1 ? VT_OK      // vt_set_template: the template's token rows are the cache; block 0 is recomputed every frame
                                   : gen_blocks(m, tokens, B, nblocks, st, feat, resid);
    if (nblocks < 0 || nblocks > m->cfg.depth) nblocks = m->cfg.depth;
    BlocksForm f;
    if (int rc = select_blocks(m, form_b(m, B), B, nblocks, zc, f0, &f)) return rc;
    if (f.tile_nt == 5) return launch_blocks_tile<5>(m, st, tokens, B, nblocks, feat, resid, zc, f0);
    if (f.tile_nt == 20) return launch_blocks_tile<20>(m, st, tokens, B, nblocks, feat, resid, zc, f0);
    const BlocksKey& k = f.frame->key;
    // the V^T low-piece scratch: only the G256 A3 form reads it, and addresses its slice's part
    const size_t vl0 = (k.NT == 20 && k.A3) ? f0 : 0;
    hipLaunchKernelGGL(f.frame->k, dim3(B), dim3(k.NW * 64), k.lds(m->cfg.depth), st, tokens, m->blocks.p, feat, resid, m->len_z, m->cfg.depth, nblocks,
                       m->sw.dbg_skip_tile, m->dbg_stamps, m->zcache.p, zc, m->blocks3.p,
                       m->vlscr.p ? reinterpret_cast<unsigned*>(m->vlscr.p) + vl0 * vlscr_floats_per_frame(m) : nullptr);
    HIP_TRY(hipGetLastError());
    return VT_OK;
}

// ---- head
// tail (optional): the tracker's map back / clip / state update / record of vt_track_step, run by the decode kernel itself
int run_decode(vt_model* m, hipStream_t st, const float* score, const float* size, const float* offset,
               const float* window, int B, float* pred, float* hann, float* conf, const TrackTail* tail = nullptr) {
    hipLaunchKernelGGL(vth::decode_kernel, dim3(B), dim3(64), 0, st, score, size, offset, window, m->F, pred, hann, conf,
                       tail ? *tail : TrackTail{}, tail ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return VT_OK;
}

// F = 16: batches up to this size run conv1 as its own launch.  SWEEP_HEAD=1 tools/small_batch_sweep.py, us per step, per-tower
// form -> split form: B=1 86.0 -> 78.6, B=8 96.6 -> 91.5, B=16 110.3 -> 103.5, B=32 135.2 -> 132.9, B=64 181.7 -> 186.2
constexpr int HEAD_SPLIT_MAX_B = 32;

struct HeadForm {      // exactly one kernel; the whole-head ones (whole, fused3, seq3) decode -- and run the tracker's tail -- themselves
    const decltype(HEAD_WHOLE)::value_type* whole = nullptr;
    const decltype(HEAD_TOWERS)::value_type* towers = nullptr;
    bool conv1 = false;      // F = 16, small batches: conv1 of every tower over four row strips (12 workgroups per frame) before `towers`
#ifndef VT_F16
    const decltype(HEAD_FUSED3)::value_type* fused3 = nullptr;
    const decltype(HEAD_TOWERS3)::value_type* towers3 = nullptr;
    const decltype(HEAD_SEQ3)::value_type* seq3 = nullptr;
#endif
};

int select_head(const vt_model* m, int Bf, int B, size_t f0, HeadForm* f) {
    const Switches& s = m->sw;
    const int F = m->F;
    if (F != 8 && F != 16) return fail(VT_ERR_ARG, "unsupported feat_sz " + std::to_string(F));
    const bool whole = s.head_fused < 0 ? Bf > 176 : s.head_fused != 0, skip = s.skip_head != 0;
#ifndef VT_F16
    if (s.head_bf3 && !skip && (F == 8 || whole)) {      // same kernel forms by batch size
        if (F == 16) f->seq3 = find_form(HEAD_SEQ3, {m->dbg_stamps != nullptr});
        else if (whole) f->fused3 = &HEAD_FUSED3[0];
        else f->towers3 = &HEAD_TOWERS3[0];
        return VT_OK;
    }
#endif
    if (whole) {
        f->whole = find_form(HEAD_WHOLE, {F, skip});
        return VT_OK;
    }
    f->conv1 = F == 16 && !skip && B <= m->head_m1_frames && f0 == 0 && (s.head_split < 0 ? Bf <= HEAD_SPLIT_MAX_B : s.head_split != 0);
    f->towers = find_form(HEAD_TOWERS, {F, skip, f->conv1});
    return VT_OK;
}

// The six outputs of the slice starting at frame f0: the caller's buffers where given, else the model's
struct OutSlice { float *score, *size, *offset, *pred, *hann, *conf; };
OutSlice out_slice(const vt_model* m, const vt_outputs* o, size_t f0) {
    const size_t n = (size_t)m->len_x;
    return {((o && o->score_map) ? o->score_map : m->score.p) + f0 * n, ((o && o->size_map) ? o->size_map : m->size.p) + f0 * 2 * n,
            ((o && o->offset_map) ? o->offset_map : m->offset.p) + f0 * 2 * n, ((o && o->pred_boxes) ? o->pred_boxes : m->pred.p) + f0 * 4,
            ((o && o->hann_boxes) ? o->hann_boxes : m->hann.p) + f0 * 4, ((o && o->conf) ? o->conf : m->conf.p) + f0};
}

int run_head(vt_model* m, const float* feat, int B, hipStream_t st, const vt_outputs* out, size_t f0 = 0, const TrackTail* tail = nullptr) {
    // outputs of the slice starting at frame f0 (feat already points at the slice)
    const OutSlice o = out_slice(m, out, f0);
    if (m->generic) {
        if (int rcg = gen_head(m, feat, B, st, o.score, o.size, o.offset)) return rcg;
        return run_decode(m, st, o.score, o.size, o.offset, m->window.p, B, o.pred, o.hann, o.conf, tail);
    }
    HeadForm f;
    if (int rc = select_head(m, form_b(m, B), B, f0, &f)) return rc;
    const TrackTail tl = tail ? *tail : TrackTail{};
    const int has_tail = tail ? 1 : 0, skip = m->sw.skip_head;
#ifndef VT_F16
    const vth3::u32x4* hw3 = reinterpret_cast<const vth3::u32x4*>(m->head3.p);
    if (f.fused3)
        hipLaunchKernelGGL(f.fused3->k, dim3(B), dim3(f.fused3->block), f.fused3->lds, st, feat, m->head.p, hw3, m->window.p, o.score, o.size, o.offset,
                           o.pred, o.hann, o.conf, tl, has_tail);
    else if (f.seq3)
        hipLaunchKernelGGL(f.seq3->k, dim3(B), dim3(f.seq3->block), f.seq3->lds, st, feat, m->head.p, hw3, m->window.p, o.score, o.size, o.offset, o.pred,
                           o.hann, o.conf, tl, has_tail, m->dbg_stamps);
    else if (f.towers3)
        hipLaunchKernelGGL(f.towers3->k, dim3(B, 3), dim3(f.towers3->block), f.towers3->lds, st, feat, m->head.p, hw3, o.score, o.size, o.offset);
    else
#endif
    if (f.whole)
        hipLaunchKernelGGL(f.whole->k, dim3(B), dim3(f.whole->block), f.whole->lds, st, feat, m->head.p, m->window.p, o.score, o.size, o.offset, o.pred,
                           o.hann, o.conf, skip, tl, has_tail);
    else {
        if (f.conv1) hipLaunchKernelGGL(vth::head_conv1_kernel<16>, dim3(4, 3, B), dim3(512), 0, st, feat, m->head.p, m->head_m1.p);
        hipLaunchKernelGGL(f.towers->k, dim3(B, 3), dim3(f.towers->block), f.towers->lds, st, f.conv1 ? m->head_m1.p : feat, m->head.p, o.score, o.size,
                           o.offset, f.conv1 ? 0 : skip);
    }
    HIP_TRY(hipGetLastError());
    bool decoded = f.towers == nullptr;       // a whole-head kernel: decoded, and the tracker's tail, if any, ran on its decoding lane
#ifndef VT_F16
    decoded = decoded && f.towers3 == nullptr;
#endif
    if (decoded) return VT_OK;
    return run_decode(m, st, o.score, o.size, o.offset, m->window.p, B, o.pred, o.hann, o.conf, tail);
}

// ViT-Base: towers + conv5 in vitb.hip, then the same decode kernel (first-index argmax, raw and Hann-windowed)
// tail: the tracker step's state tail on the decode kernel's lane (the WHOLE batch's: a slice addresses it from its frame f0 here)
int run_head_vitb(vt_model* m, const float* feat, int B, hipStream_t st, const vt_outputs* out, const vb::Slice* sl = nullptr,
                  const TrackTail* tail = nullptr) {
    const size_t f0 = sl ? sl->f0 : 0;
    const OutSlice o = out_slice(m, out, f0);
    std::string err;
    int rc = vb::head(m->vb, feat, B, st, o.score, o.size, o.offset, &err, sl);
    if (rc) return fail(rc, err);
    if (!tail) return run_decode(m, st, o.score, o.size, o.offset, m->window.p, B, o.pred, o.hann, o.conf);
    TrackTail t = *tail;
    t.resize_factor += f0;
    t.states += 4 * f0;
    if (t.record) t.record += 5 * f0;
    if (t.frames) t.frames += f0;
    return run_decode(m, st, o.score, o.size, o.offset, m->window.p, B, o.pred, o.hann, o.conf, &t);
}

// -------------------------------------------------------------------------------------------- step
// Steps on the cached template need it for every frame of the batch -- and, on the vit_48 paths (forms = true), written under the
// form batch of this call: the cache holds the operands of THAT form's block 0.
int check_template_cache(const vt_model* m, int B, const char* who, bool forms) {
    if (m->tmpl_frames < B)
        return fail(VT_ERR_STATE, std::string(who) + " on the cached (null) template needs vt_set_template for at least " + std::to_string(B) + " frames first");
    if (forms && m->tmpl_form_batch != m->form_batch)
        return fail(VT_ERR_STATE, "the template cache was written under another form batch: call vt_set_template again after vt_set_form_batch");
    return VT_OK;
}

// vit_48: the frames [f0, f0 + nb) of a batch through stem + blocks + head on stream st.  z: the template crops of the WHOLE batch, or null:
// the cached template (vt_set_template; not sliced).  x: the search crops of the whole batch, fp32 (B, 3, Tx, Tx) or, xu8, uint8 patches
// (B, Tx, Tx, 3).  tail (optional): the tracker step's state update, on the head's decoding lane.
int vt48_network(vt_model* m, const float* z, const float* x, bool xu8, size_t f0, int nb, hipStream_t st, const vt_outputs* out,
                 const TrackTail* tail = nullptr) {
    const size_t Tz = m->cfg.template_size, Tx = m->cfg.search_size, C = (size_t)m->cfg.channels;
    // the cached step has a token matrix of its own: its template rows are written by vt_set_template only
    float* const tok = (z ? m->tokens.p : m->tokens_c.p) + f0 * m->L * C;
    float* const feat = m->feat.p + f0 * m->len_x * C;
    const float* const xs = x + f0 * 3 * Tx * Tx / (xu8 ? sizeof(float) : 1);
    int rc;
    if (!z) rc = run_stem(m, nullptr, xs, nb, st, tok, f0, 1, xu8);      // block 0 loads the template's q / k / v
    else if (!xu8) rc = run_stem(m, z + f0 * 3 * Tz * Tz, xs, nb, st, tok, f0);
    else if (!(rc = run_stem(m, z + f0 * 3 * Tz * Tz, nullptr, nb, st, tok, f0, 2)))      // the template's rows from the fp32 crop, ...
        rc = run_stem(m, nullptr, xs, nb, st, tok, f0, 1, true);                           // ... the search rows from the patch
    if (rc || (rc = run_blocks(m, tok, nb, -1, st, feat, nullptr, z ? 0 : 2, f0))) return rc;
    return run_head(m, feat, nb, st, out, f0, tail);
}

// vt_set_template's stages: the template token rows (stem(z) + pos_embed_z) of n frames into `tokens`, and block 0's LN1 + qkv of those rows
// into the cache.  One block over the whole token matrix: the search rows hold whatever the last frame left (per-token work, nothing of
// theirs is stored); the outputs are scratch.
int vt48_template_rows(vt_model* m, const float* z, int n, hipStream_t st, float* tokens) {
    if (int rc = run_stem(m, z, nullptr, n, st, tokens, 0, 2)) return rc;
    return run_blocks(m, tokens, n, 1, st, m->feat.p, nullptr, 1);
}

// ViT-Base: stem on the given / cached template + blocks + head of the frames [f0, f0 + nb) of a batch of Btot, on stream st
int vitb_network(vt_model* m, vb::ZSrc zsrc, const float* z, const float* x, const unsigned char* xu8, size_t f0, int nb, int Btot, int cus,
                 hipStream_t st, const vt_outputs* out, const TrackTail* tail) {
    const size_t Tz = m->cfg.template_size, Tx = m->cfg.search_size;
    const vb::Slice sl{f0, Btot, cus};
    std::string err;
    int rc;
    if (zsrc == vb::Z_GIVEN && x)      // both crops as fp32: one patch GEMM over all token rows
        rc = vb::stem(m->vb, z + f0 * 3 * Tz * Tz, x + f0 * 3 * Tx * Tx, nb, st, nullptr, &err, &sl);
    else
        rc = vb::stem_rows(m->vb, zsrc, z ? z + f0 * 3 * Tz * Tz : nullptr, x ? x + f0 * 3 * Tx * Tx : nullptr, xu8 ? xu8 + f0 * 3 * Tx * Tx : nullptr, nb, st,
                           nullptr, &err, &sl);
    if (rc || (rc = vb::blocks(m->vb, nullptr, nb, -1, st, nullptr, nullptr, &err, &sl))) return fail(rc, err);
    return run_head_vitb(m, nullptr, nb, st, out, &sl, tail);
}

// ---- chains: frame slices of one step as concurrent chains (VT_GRAPH_CHAINS; read_switches)
int chain_count(const vt_model* m, int B) {
    int nch = m->sw.graph_chains;
    if (nch == 0) nch = (m->vb && B >= 64) ? 2 : 1;      // auto (the ViT-Base default): two chains from 64 frames up
    return std::max(1, std::min({nch, 4, B}));
}

// ViT-Base: the CUs each of nch chains' persistent GEMMs launch on -- all of them under the automatic choice, else an equal share (VT_CHAIN_CUS: that many)
int chain_cus(const vt_model* m, int nch) {
    int ncu = 256;
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0);
    return m->sw.chain_cus > 0 ? m->sw.chain_cus : (m->sw.graph_chains == 0 ? ncu : ncu / nch);
}

// slice(c, f0, nb, stream) for each of nch slices of B frames: chain 0 on `st`, the others forked off it onto the side streams and joined back
// with events, which is legal under stream capture and in eager mode.  Frames are independent, so the chains compute what one chain
// computes, bit for bit.
template <class F> int fork_join(vt_model* m, hipStream_t st, int nch, int B, F&& slice) {
    if (nch == 1) return slice(0, (size_t)0, B, st);
    if (hipEventRecord(m->fork_ev, st) != hipSuccess) return fail(VT_ERR_HIP, "hipEventRecord(fork)");
    int rc = VT_OK;
    for (int c = 1; c < nch && !rc; ++c)
        if (hipStreamWaitEvent(m->side_stream[c - 1], m->fork_ev, 0) != hipSuccess) rc = fail(VT_ERR_HIP, "hipStreamWaitEvent(fork)");
    for (int c = 0; c < nch && !rc; ++c) {
        const size_t f0 = (size_t)B * c / nch, f1 = (size_t)B * (c + 1) / nch;
        rc = slice(c, f0, (int)(f1 - f0), c == 0 ? st : m->side_stream[c - 1]);
    }
    for (int c = 1; c < nch; ++c) {   // always join, even after an error, so that a capture can end
        (void)hipEventRecord(m->join_ev[c - 1], m->side_stream[c - 1]);
        (void)hipStreamWaitEvent(st, m->join_ev[c - 1], 0);
    }
    return rc;
}

// The ViT-Base step as ONE chain, or from 64 frames up as chains (the tracker step inside a caller's graph, vt_forward_u8, a captured step)
int vitb_network_chains(vt_model* m, int nch, vb::ZSrc zsrc, const float* z, const float* x, const unsigned char* xu8, int B, hipStream_t st,
                        const vt_outputs* out, const TrackTail* tail) {
    const int cus = nch == 1 ? 0 : chain_cus(m, nch);
    return fork_join(m, st, nch, B, [&](int, size_t f0, int nb, hipStream_t cs) { return vitb_network(m, zsrc, z, x, xu8, f0, nb, B, cus, cs, out, tail); });
}

// ---- crop: which kernel form this device can run
// crop_kernel<false> fetches a bilinear sample's two RGB pixels with ONE 8-byte buffer load at byte offset 3 x: it relies on the
// device serving byte-unaligned dword loads and on out-of-range buffer reads returning zero (tools/src/probe_unaligned.hip).  Neither
// is architectural, so the first vt_create of a process crops a known frame with both forms -- device memory and device-mapped pinned
// host memory (the plugin's zero-copy frames) -- and falls back to the byte-load form on any difference (round 3 advisor).
// The decision is per DEVICE (a process may drive several), taken once under a mutex by whichever vt_create or vt_crop gets there
// first -- ViT-Base models included (round 4 advisor).
constexpr int CROP_MAX_DEVICES = 64;
int g_crop_bytes[CROP_MAX_DEVICES];        // 0: not tested yet, 1: fast form, 2: byte-load form
std::mutex g_crop_mutex;

// The kernel of each crop form: the dense one, or its frame-table twin (vt_track.h: the same body on TableFrames)
template <bool TB, bool BYTES, bool U8> constexpr auto crop_k() {
    if constexpr (TB) return &vtt::crop_frames_kernel<BYTES, U8>; else return &vtt::crop_kernel<BYTES, U8>;
}
template <bool TB, int G, bool U8> constexpr auto crop_fast_k() {
    if constexpr (TB) return &vtt::crop_fast_frames_kernel<G, U8>; else return &vtt::crop_fast_kernel<G, U8>;
}
template <bool TB, bool U8, int LG, int IPT, bool AL> constexpr auto crop_band_k() {
    if constexpr (TB) return &vtt::crop_band_kernel<U8, LG, IPT, AL, vtt::TableFrames>; else return &vtt::crop_band_kernel<U8, LG, IPT, AL>;
}

// Where the crop reads from: dense frames (B, H, W, 3), a (B,) vt_frame table (H / W unused), or a (B,) vt_image table (vt_crop_images & co.;
// sizes: null, or a (B,) vt_frame table that receives each descriptor's H and W for the tracker tail's clip)
struct CropSrc {
    const unsigned char* frames = nullptr;
    int H = 0, W = 0;
    const vt_frame* table = nullptr;
    const vt_image* images = nullptr;
    vt_frame* sizes = nullptr;
    const void* ptr() const { return images ? (const void*)images : table ? (const void*)table : (const void*)frames; }
};

// The tracker's sizes: crop_band_kernel / crop_band_image_kernel (a workgroup owns a band of VT_CROP_BAND x 256 items) when its bands fill the
// chip.  A thread of a band walks its items one after the other, so a few frames are a long dependent chain on a few CUs: one frame at
// T = 128 takes 12.1 us as four bands of four items, 8.0 as eight bands of two, 5.4 as sixteen workgroups of crop_fast_kernel
// (tools/gpu_b1prof.sh) -- the form follows the number of workgroups the batch gives each CU.
// Returns the items per thread (4 or 2), or 0: no band form for this call.
int crop_band_ipt(int B, int T, bool u8out) {
    const CropSwitches& c = crop_switches();
    const long items = (long)B * T * (T / 4);
    // at least one two-item band (512 items) per CU; VT_CROP_BAND=-4 / -2 force a band form (tests)
    if (c.band == 0 || !(c.band < 0 || items >= 2L * 256 * 256) || !(T == 64 || T == 128 || T == 256)) return 0;
    // the fp32 form (template crops, VT_TRACK_U8=0, ViT-Base) keeps a normalised float4 per channel and item: two items per thread measure
    // 17.3 against 18.0 us (T = 128) and 51.7 against 55.5 (T = 256) for 256 frames; an explicit VT_CROP_BAND decides for both forms
    if (!u8out && !c.band_set) return 2;
    return ((c.band >= 4 || c.band <= -4) && !(c.band > 0 && items < 4L * 256 * 256)) ? 4 : 2;
}
// f(U8, LGT4, IPT as integral constants) for the band form of a call
template <class F> void crop_band_dispatch(bool u8out, int T, int ipt, F&& f) {
    auto by_ipt = [&](auto u8c, auto lgc) {
        if (ipt == 4) f(u8c, lgc, std::integral_constant<int, 4>{});
        else f(u8c, lgc, std::integral_constant<int, 2>{});
    };
    auto by_size = [&](auto u8c) {
        if (T == 64) by_ipt(u8c, std::integral_constant<int, 4>{});
        else if (T == 128) by_ipt(u8c, std::integral_constant<int, 5>{});
        else by_ipt(u8c, std::integral_constant<int, 6>{});
    };
    if (u8out) by_size(std::true_type{});
    else by_size(std::false_type{});
}

// u8out: `crops` is a uint8 (B, T, T, 3) patch buffer (sample_target's output; mean3 / std3 unused) instead of the fp32 (B, 3, T, T) crop
// TB (a std::bool_constant): `frames` is a (B,) vt_frame table (vt_crop_frames; H / W unused) and every form below runs its frame-table
// twin, chosen by the same rules as the dense form
template <class TBc>
void launch_crop_forms(TBc, bool bytes, const unsigned char* frames, int H, int W, const double* states, double factor, int T,
                       const float* mean3, const float* std3, int B, hipStream_t st, float* crops, double* rf, bool u8out) {
    constexpr bool TB = TBc::value;
    const CropSwitches& cs = crop_switches();
    const int ipt = (!bytes && cs.fast > 0) ? crop_band_ipt(B, T, u8out) : 0;
    if (ipt) {
        crop_band_dispatch(u8out, T, ipt, [&](auto u8c, auto lgc, auto iptc) {
            constexpr bool U = decltype(u8c)::value;
            constexpr int LG = decltype(lgc)::value, IPT = decltype(iptc)::value;
            auto go = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, dim3(T * (T / 4) / (256 * IPT), B), dim3(256), 0, st, frames, H, W, states, factor, mean3[0], mean3[1], mean3[2],
                                   std3[0], std3[1], std3[2], crops, rf);
            };
            if (cs.aligned) go(crop_band_k<TB, U, LG, IPT, true>());
            else go(crop_band_k<TB, U, LG, IPT, false>());
        });
        return;
    }
    if (!bytes && cs.fast > 0 && (T & 3) == 0 && T <= vtt::CROP_FAST_MAX_T) {
        const int ngroups = (T * (T / 4) + 255) / 256;
        auto go = [&](auto u8c, auto g) {
            constexpr int G = decltype(g)::value;
            hipLaunchKernelGGL((crop_fast_k<TB, G, decltype(u8c)::value>()), dim3((ngroups + G - 1) / G, B), dim3(256), 0, st, frames, H, W, states, factor, T,
                               mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], crops, rf);
        };
        if (u8out) go(std::true_type{}, std::integral_constant<int, 1>{});
        else if (cs.fast >= 4 && ngroups >= 4) go(std::false_type{}, std::integral_constant<int, 4>{});
        else if (cs.fast >= 2 && ngroups >= 2) go(std::false_type{}, std::integral_constant<int, 2>{});
        else go(std::false_type{}, std::integral_constant<int, 1>{});
        return;
    }
    auto go = [&](auto bytesc, auto u8c) {
        hipLaunchKernelGGL((crop_k<TB, decltype(bytesc)::value, decltype(u8c)::value>()), dim3((T * ((T + 3) / 4) + 255) / 256, B), dim3(256), 0, st, frames, H,
                           W, states, factor, T, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], crops, rf);
    };
    if (u8out) bytes ? go(std::true_type{}, std::true_type{}) : go(std::false_type{}, std::true_type{});
    else bytes ? go(std::true_type{}, std::false_type{}) : go(std::false_type{}, std::false_type{});
}

// The crop of any source.  bytes: the device needs the byte-load form (crop_selftest).  The forms on a vt_image table depend on the
// device's unaligned-access mode in neither form (dword-aligned windows, or single bytes), so the self test's choice does not apply to them.
void launch_crop(bool bytes, const CropSrc& src, const double* states, double factor, int T, const float* mean3, const float* std3, int B,
                 hipStream_t st, float* crops, double* rf, bool u8out) {
    static const float none3[3] = {0.f, 1.f, 1.f};      // a patch is not normalised: its kernels ignore mean and std
    if (u8out) mean3 = std3 = none3;
    if (src.table)
        return launch_crop_forms(std::true_type{}, bytes, reinterpret_cast<const unsigned char*>(src.table), 0, 0, states, factor, T, mean3, std3, B, st,
                                 crops, rf, u8out);
    if (!src.images) return launch_crop_forms(std::false_type{}, bytes, src.frames, src.H, src.W, states, factor, T, mean3, std3, B, st, crops, rf, u8out);
    if (const int ipt = crop_band_ipt(B, T, u8out)) {
        crop_band_dispatch(u8out, T, ipt, [&](auto u8c, auto lgc, auto iptc) {
            constexpr int IPT = decltype(iptc)::value;
            hipLaunchKernelGGL((vtt::crop_band_image_kernel<decltype(u8c)::value, decltype(lgc)::value, IPT>), dim3(T * (T / 4) / (256 * IPT), B), dim3(256), 0,
                               st, src.images, src.sizes, states, factor, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], crops, rf);
        });
        return;
    }
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((T * ((T + 3) / 4) + 255) / 256, B), dim3(256), 0, st, src.images, src.sizes, states, factor, T, mean3[0], mean3[1],
                           mean3[2], std3[0], std3[1], std3[2], crops, rf);
    };
    if (u8out) go(&vtt::crop_image_kernel<true>);
    else go(&vtt::crop_image_kernel<false>);
}

// device buffers of the self test, released on every path
struct CropProbe {
    unsigned char *dfr = nullptr, *hfr = nullptr;
    double *dst = nullptr, *drf = nullptr;
    float* dout = nullptr;
    ~CropProbe() {
        if (dfr) (void)hipFree(dfr);
        if (hfr) (void)hipHostFree(hfr);
        if (dst) (void)hipFree(dst);
        if (drf) (void)hipFree(drf);
        if (dout) (void)hipFree(dout);
    }
};

// *bytes_form = whether the current device needs the byte-load form
int crop_selftest(bool* bytes_form = nullptr) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= CROP_MAX_DEVICES) return fail(VT_ERR_ARG, "device index beyond the crop self test's table");
    std::lock_guard<std::mutex> lock(g_crop_mutex);
    if (g_crop_bytes[dev] == 0) {
        constexpr int H = 13, W = 17, T = 20, B = 2;          // odd sizes: windows at every byte alignment, crops across all four borders
        std::vector<unsigned char> fr((size_t)B * H * W * 3);
        for (size_t i = 0; i < fr.size(); ++i) fr[i] = (unsigned char)((i * 131u + (i >> 3) * 17u + 7u) & 0xffu);
        const double st[B * 4] = {-2.5, -1.5, 9.0, 8.0, 9.5, 6.25, 9.0, 8.5};      // one box over the top-left corner, one over the bottom-right
        const float mean3[3] = {0.485f, 0.456f, 0.406f}, std3[3] = {0.229f, 0.224f, 0.225f};
        CropProbe b;
        const size_t nout = (size_t)B * 3 * T * T;
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&b.dfr), fr.size()));
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&b.hfr), fr.size(), hipHostMallocMapped));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&b.dst), sizeof(st)));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&b.drf), B * sizeof(double)));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&b.dout), 3 * nout * sizeof(float)));
        HIP_TRY(hipMemcpy(b.dfr, fr.data(), fr.size(), hipMemcpyHostToDevice));
        std::memcpy(b.hfr, fr.data(), fr.size());
        HIP_TRY(hipMemcpy(b.dst, st, sizeof(st), hipMemcpyHostToDevice));
        launch_crop(true, CropSrc{b.dfr, H, W}, b.dst, 2.0, T, mean3, std3, B, nullptr, b.dout, b.drf, false);                  // the reference form
        launch_crop(false, CropSrc{b.dfr, H, W}, b.dst, 2.0, T, mean3, std3, B, nullptr, b.dout + nout, b.drf, false);          // fast form, device memory
        launch_crop(false, CropSrc{b.hfr, H, W}, b.dst, 2.0, T, mean3, std3, B, nullptr, b.dout + 2 * nout, b.drf, false);      // fast form, pinned host memory
        HIP_TRY(hipGetLastError());
        std::vector<float> out(3 * nout);
        HIP_TRY(hipMemcpy(out.data(), b.dout, out.size() * sizeof(float), hipMemcpyDeviceToHost));
        const bool same = std::memcmp(out.data(), out.data() + nout, nout * sizeof(float)) == 0 &&
                          std::memcmp(out.data(), out.data() + 2 * nout, nout * sizeof(float)) == 0;
        const int forced = crop_switches().bytes;     // VT_CROP_BYTES: force a form (tests)
        g_crop_bytes[dev] = forced >= 0 ? (forced ? 2 : 1) : (same ? 1 : 2);
    }
    if (bytes_form) *bytes_form = g_crop_bytes[dev] == 2;
    return VT_OK;
}

// The six exported crop functions and the tracker step's crop: argument check, the device's crop form, launch.  mean3 / std3: of the fp32
// crop; u8out: `out` is a uint8 patch buffer instead, which the kernels write as 12-byte pixel groups through 4-byte-aligned pointers.
int run_crop(const vt_model* m, const CropSrc& src, const double* states, double factor, int T, const float* mean3, const float* std3, int B,
             void* stream, void* out, double* rf, bool u8out) {
    if (!m || !src.ptr() || !states || !out || !rf || (!u8out && (!mean3 || !std3))) return fail(VT_ERR_ARG, "null argument");
    if (B < 1 || T < 1 || !(factor > 0.0) || (src.frames && (src.H < 1 || src.W < 1))) return fail(VT_ERR_ARG, "bad crop arguments");
    if (u8out && (reinterpret_cast<uintptr_t>(out) & 3)) return fail(VT_ERR_ARG, "the uint8 patch buffer must be 4-byte aligned");
    bool bytes = false;
    if (!src.images)
        if (int rc = crop_selftest(&bytes)) return rc;      // a table look-up after the device's first call
    launch_crop(bytes, src, states, factor, T, mean3, std3, B, static_cast<hipStream_t>(stream), static_cast<float*>(out), rf, u8out);
    HIP_TRY(hipGetLastError());
    return VT_OK;
}

// What every model kind has: geometry, switches, the output buffers, the Hann window, the capture stream and the chains' streams and events.
// The first error is returned; the caller destroys the model.
int init_model(vt_model* m, const vt_config* cfg, bool vitb) {
    m->cfg = *cfg;
    m->sw = read_switches(*cfg, vitb);
    m->F = cfg->search_size / 16;
    m->Fz = cfg->template_size / 16;
    m->len_x = m->F * m->F;
    m->len_z = m->Fz * m->Fz;
    m->L = m->len_x + m->len_z;
    const size_t B = (size_t)cfg->max_batch, n = (size_t)m->len_x;
    const std::pair<DevBuf*, size_t> bufs[] = {{&m->score, B * n}, {&m->size, B * 2 * n}, {&m->offset, B * 2 * n}, {&m->pred, B * 4}, {&m->hann, B * 4},
                                               {&m->conf, B}, {&m->imsizes, B * sizeof(vt_frame) / sizeof(float)}};      // imsizes: vt_track_step_images
    for (const auto& b : bufs)
        if (int rc = b.first->alloc(b.second)) return rc;
    if (int rc = upload(m->window, hann2d(m->F))) return rc;
    if (hipStreamCreateWithFlags(&m->cap_stream, hipStreamNonBlocking) != hipSuccess) return fail(VT_ERR_HIP, "hipStreamCreate failed");
    for (int i = 0; i < 3; ++i)
        if (hipStreamCreateWithFlags(&m->side_stream[i], hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&m->join_ev[i], hipEventDisableTiming) != hipSuccess)
            return fail(VT_ERR_HIP, "hipStreamCreate / hipEventCreate failed");
    if (hipEventCreateWithFlags(&m->fork_ev, hipEventDisableTiming) != hipSuccess) return fail(VT_ERR_HIP, "hipEventCreate failed");
    return VT_OK;
}

// ViT-Base or ViT-Large model: the shared part of vt_model is the output scratch, the window and the streams
int create_vitb(const vt_config* cfg, vt_model** out, bool family_vit = false) {
    std::string err;
    VbModel* vbm = nullptr;
    int rc = family_vit ? vb::create_vit(cfg, &vbm, &err) : vb::create(cfg, &vbm, &err);
    if (rc) return fail(rc, err);
    if ((rc = crop_selftest())) { vb::destroy(vbm); return rc; }      // every model kind can be handed to vt_crop (after the argument checks: they need no device)
    vt_model* m = new vt_model();
    m->vb = vbm;
    if ((rc = init_model(m, cfg, true))) { vt_destroy(m); return rc; }
    if (const char* p = std::getenv("VB_PRECISION"); p && *p) {      // the mode from the start, where no call chooses one (vt_set_precision)
        const std::string v(p);
        if (v != "fp32" && v != "bf16") { vt_destroy(m); return fail(VT_ERR_ARG, "VB_PRECISION=" + v + ": bf16 or fp32"); }
        if (v == "fp32" && (rc = vb::set_precision(m->vb, VT_PRECISION_FP32, &err))) { vt_destroy(m); return fail(rc, err); }
    }
    *out = m;
    return VT_OK;
}

}  // namespace

// =========================================================================================== ABI
extern "C" {

const char* vt_last_error(void) { return g_err.c_str(); }
const char* vt_version(void) { return "vittrack-hip 0.2 (gfx950, " VT_PRECISION_NAME " contractions)"; }

int vt_create_vit(const vt_config* cfg, vt_model** out) {
    if (!cfg || !out) return fail(VT_ERR_ARG, "null argument");
    return create_vitb(cfg, out, true);
}

int vt_create(const vt_config* cfg, vt_model** out) {
    if (!cfg || !out) return fail(VT_ERR_ARG, "null argument");
    if (cfg->channels == 768) return create_vitb(cfg, out);
    // ViT-Large OSTrack: this exact tuple leaves the shape-generic surface for the bf16 path of vitb.hip (which checks the depth); every other
    // 1024-wide configuration goes on below
    if (cfg->channels == 1024 && cfg->heads == 16 && cfg->head_channels == 256 && cfg->stride == 16 &&
        ((cfg->template_size == 128 && cfg->search_size == 256) || (cfg->template_size == 192 && cfg->search_size == 384)))
        return create_vitb(cfg, out);
    // build_ostrack_dist takes embed_dim / num_heads / the head width from the YAML (vit_dist.py:159-164; head.py:352-359): the shipped widths
    // (48, 1, 32) at the two geometries of the repository's configs run the tuned kernels, everything else the shape-generic ones
    const bool shipped_widths = cfg->channels == 48 && cfg->heads == 1 && cfg->head_channels == 32;
    if (cfg->stride != 16 || cfg->channels < 8 || cfg->channels > 1024 || cfg->channels % 8 != 0 || cfg->heads < 1 || cfg->channels % cfg->heads != 0 ||
        cfg->channels / cfg->heads > vtg::MAXHD || cfg->head_channels < 8 || cfg->head_channels > 1024 || cfg->head_channels % 8 != 0)
        return fail(VT_ERR_ARG,
                    "unsupported model: STRIDE must be 16, CHANNELS a multiple of 8 (the stem's widths are C/8, C/4, C/2, C) divisible by HEADS with a head "
                    "dimension of at most " + std::to_string(vtg::MAXHD) + ", HEAD.NUM_CHANNELS a multiple of 8 (the towers' widths are W, W/2, W/4, W/8); "
                    "got channels=" + std::to_string(cfg->channels) + " heads=" + std::to_string(cfg->heads) + " head_channels=" + std::to_string(cfg->head_channels) +
                    " stride=" + std::to_string(cfg->stride));
    const bool g128 = shipped_widths && cfg->template_size == 64 && cfg->search_size == 128;
    const bool g256 = shipped_widths && cfg->template_size == 128 && cfg->search_size == 256;
    const bool generic = !g128 && !g256;
    if (generic && (cfg->template_size % 16 != 0 || cfg->search_size % 16 != 0 || cfg->template_size < 16 || cfg->search_size < 16 ||
                    cfg->template_size > 512 || cfg->search_size > 512))
        return fail(VT_ERR_ARG, "unsupported geometry (template,search)=(" + std::to_string(cfg->template_size) + "," +
                                    std::to_string(cfg->search_size) + "): sizes must be multiples of 16 in [16, 512]; tuned kernels exist for (64,128) and "
                                    "(128,256), every other size runs the shape-generic kernels");
    if (cfg->depth < 1 || cfg->depth > 12 || cfg->max_batch < 1) return fail(VT_ERR_ARG, "bad depth / max_batch");
    if (!generic) {   // the block kernel keeps every block's LayerNorm vectors and biases in LDS next to the K/V images
        const size_t need = g128 ? blocks_lds_bytes(5, true, true, cfg->depth) : blocks_lds_bytes(20, false, false, cfg->depth);
        if (need > LDS_PER_CU)
            return fail(VT_ERR_ARG, "depth " + std::to_string(cfg->depth) + " needs " + std::to_string(need) +
                                        " B of LDS per workgroup at this geometry (limit " + std::to_string(LDS_PER_CU) + ")");
    }

    if (int rcs = crop_selftest()) return rcs;
    vt_model* m = new vt_model();
    int rc = init_model(m, cfg, false);
    const size_t B = (size_t)cfg->max_batch;
    auto A = [&](DevBuf& d, size_t n) { if (!rc) rc = d.alloc(n); };
    m->generic = generic;
    m->gd = vtg::Dims{cfg->channels, cfg->heads, cfg->head_channels};
    const size_t C = (size_t)cfg->channels, HW = (size_t)cfg->head_channels;
    A(m->tokens, B * m->L * C);
    A(m->feat, B * m->len_x * C);
    A(m->tokens_c, B * m->L * C);
    if (generic) {
        const size_t T = (size_t)std::max(cfg->search_size, cfg->template_size);
        // ping-pong maps: stem layers 1 / 3 and head convs 1 / 3 in g_a, layers 2 and convs 2 / 4 in g_b
        A(m->g_a, std::max({B * (C / 8) * (T / 2) * (T / 2), B * (C / 2) * (T / 8) * (T / 8), 3 * B * (size_t)m->len_x * HW}));
        A(m->g_b, std::max(B * (C / 4) * (T / 4) * (T / 4), 3 * B * (size_t)m->len_x * (HW / 2)));
        A(m->g_qkv, B * m->L * 3 * C);
        A(m->g_ao, B * m->L * C);
        A(m->g_hid, B * m->L * 4 * C);
        A(m->g_x, B * m->L * C);
    } else {
    A(m->act_x, B * (size_t)(cfg->search_size / 4) * (cfg->search_size / 4) * 12);
    A(m->act_z, B * (size_t)(cfg->template_size / 4) * (cfg->template_size / 4) * 12);
    A(m->zcache, B * (size_t)(m->len_z / 16) * 9 * 256);
    if (m->L / 16 == 20 && !VT_IS_F16) A(m->vlscr, B * vlscr_floats_per_frame(m));      // (the f16 build's block kernels keep V^T as one f16 image)
    m->tile_frames = (int)std::min<size_t>(B, 128);
    A(m->tile_q, 2 * (size_t)m->tile_frames * m->L * 48);      // two sets each (launch_blocks_tile)
    A(m->tile_k, 2 * (size_t)m->tile_frames * m->L * 48);
    A(m->tile_v, 2 * (size_t)m->tile_frames * m->L * 48);
    A(m->tile_x, (size_t)m->tile_frames * m->L * 48);
    }
    if (!generic && m->F == 16) {
        m->head_m1_frames = (int)std::min<size_t>(B, 176);
        A(m->head_m1, (size_t)m->head_m1_frames * 3 * 8 * vth::Geo<16>::NPIX * 4);
        if (!rc && hipMemset(m->head_m1.p, 0, m->head_m1.n * sizeof(float)) != hipSuccess) rc = fail(VT_ERR_HIP, "hipMemset(head_m1) failed");
    }
    if (!rc && hipMemset(m->tokens_c.p, 0, m->tokens_c.n * sizeof(float)) != hipSuccess) rc = fail(VT_ERR_HIP, "hipMemset(tokens) failed");
    if (!generic) {
        const StemPlan sx = stem_plan(cfg->search_size), sz = stem_plan(cfg->template_size);
        m->plan_r2[0] = sx.r2; m->plan_r4[0] = sx.r4; m->plan_r2[1] = sz.r2; m->plan_r4[1] = sz.r4;
    }
    if (!rc && m->sw.dbg_stamps) {
        if (hipMalloc(reinterpret_cast<void**>(&m->dbg_stamps), B * 8 * 64 * sizeof(unsigned long long)) != hipSuccess)
            rc = fail(VT_ERR_HIP, "hipMalloc(stamps) failed");
    }
    if (!rc) {      // the dynamic-LDS opt-in of every form the selectors can return, at exactly the size it is launched with
        hipError_t e = hipSuccess;
        for_each_lds_form(m, [&](const void* kernel, size_t bytes) {
            if (e == hipSuccess) e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        });
        if (e != hipSuccess) rc = fail(VT_ERR_HIP, std::string("hipFuncSetAttribute: ") + hipGetErrorString(e));
    }
    if (rc) {
        vt_destroy(m);
        return rc;
    }
    *out = m;
    return VT_OK;
}

void vt_destroy(vt_model* m) {
    if (!m) return;
    for (vt_graph* g : m->graphs) g->owner = nullptr;      // graphs that outlive their model must not reach into it (they may still be destroyed)
    m->graphs.clear();
    if (m->vb) vb::destroy(m->vb);
    for (int i = 0; i < 4; ++i) { m->stem_w[i].release(); m->stem_b[i].release(); }
    m->stem_w2k.release();
    m->stem_w1u.release();
    m->stem_w3b.release();
    m->stem_w4b.release();
    m->act_x.release(); m->act_z.release();
    DevBuf* all[] = {&m->pos_z, &m->pos_x, &m->blocks, &m->blocks3, &m->head, &m->head3, &m->window, &m->tokens, &m->feat, &m->zcache, &m->zstage, &m->imsizes, &m->vlscr, &m->tokens_c,
                     &m->tile_q, &m->tile_k, &m->tile_v, &m->tile_x, &m->head_m1,
                     &m->score, &m->size, &m->offset, &m->pred, &m->hann, &m->conf};
    for (DevBuf* d : all) d->release();
    for (int i = 0; i < 4; ++i) { m->g_stem_w[i].release(); m->g_stem_b[i].release(); }
    DevBuf* gen[] = {&m->g_blocks, &m->g_head, &m->g_a, &m->g_b, &m->g_qkv, &m->g_ao, &m->g_hid, &m->g_x};
    for (DevBuf* d : gen) d->release();
    if (m->cap_stream) (void)hipStreamDestroy(m->cap_stream);
    for (int i = 0; i < 3; ++i) {
        if (m->side_stream[i]) (void)hipStreamDestroy(m->side_stream[i]);
        if (m->join_ev[i]) (void)hipEventDestroy(m->join_ev[i]);
    }
    if (m->fork_ev) (void)hipEventDestroy(m->fork_ev);
    if (m->dbg_stamps) (void)hipFree(m->dbg_stamps);
    delete m;
}

int vt_load_weights(vt_model* m, const vt_tensor* tensors, int32_t n) {
    if (!m || !tensors || n < 0) return fail(VT_ERR_ARG, "null argument");
    TensorMap tm;
    for (int i = 0; i < n; ++i)
        if (tensors[i].name && tensors[i].data) tm[tensors[i].name] = {tensors[i].data, tensors[i].numel};
    if (m->vb) {
        std::string err;
        if (int rc = vb::load_weights(m->vb, tm, &err)) return fail(rc, err);
        m->weights_loaded = true;
        return VT_OK;
    }
    return m->generic ? load_weights_generic(m, tm) : load_weights_tuned(m, tm);
}

int vt_set_window(vt_model* m, const float* host_window) {
    if (!m || !host_window) return fail(VT_ERR_ARG, "null argument");
    return upload(m->window, std::vector<float>(host_window, host_window + (size_t)m->F * m->F));
}

int vt_set_form_batch(vt_model* m, int32_t n) {
    if (!m) return fail(VT_ERR_ARG, "null model");
    if (n < 0) return fail(VT_ERR_ARG, "vt_set_form_batch: n must be >= 0 (0 = choose the kernel forms by each call's own batch)");
    if (n != m->form_batch && m->graphs_captured > 0)
        return fail(VT_ERR_STATE, "vt_set_form_batch after vt_graph_capture: the captured graphs keep the forms of their capture -- set the form "
                                  "batch before capturing (or use a fresh model)");
    m->form_batch = n;
    return VT_OK;
}

int vt_query(const vt_model* m, int32_t* len_z, int32_t* len_x, int32_t* feat_sz, int32_t* channels) {
    if (!m) return fail(VT_ERR_ARG, "null model");
    if (len_z) *len_z = m->len_z;
    if (len_x) *len_x = m->len_x;
    if (feat_sz) *feat_sz = m->F;
    if (channels) *channels = m->cfg.channels;
    return VT_OK;
}

int vt_stem(vt_model* m, const float* z_dev, const float* x_dev, int32_t B, void* stream, float* tokens_dev) {
    int rc = check_ready(m, B);
    if (rc) return rc;
    if (!z_dev || !x_dev || !tokens_dev) return fail(VT_ERR_ARG, "null device pointer");
    if (m->vb) {
        std::string err;
        rc = vb::stem(m->vb, z_dev, x_dev, B, static_cast<hipStream_t>(stream), tokens_dev, &err);
        return rc ? fail(rc, err) : VT_OK;
    }
    return run_stem(m, z_dev, x_dev, B, static_cast<hipStream_t>(stream), tokens_dev);
}

int vt_blocks(vt_model* m, const float* tokens_dev, int32_t B, int32_t nblocks, void* stream, float* feat_dev,
              float* resid_dev) {
    int rc = check_ready(m, B);
    if (rc) return rc;
    if (!tokens_dev) return fail(VT_ERR_ARG, "null device pointer");
    if (m->vb) {
        std::string err;
        rc = vb::blocks(m->vb, tokens_dev, B, nblocks, static_cast<hipStream_t>(stream), feat_dev, resid_dev, &err);
        return rc ? fail(rc, err) : VT_OK;
    }
    return run_blocks(m, tokens_dev, B, nblocks, static_cast<hipStream_t>(stream), feat_dev ? feat_dev : m->feat.p,
                      resid_dev);
}

int vt_head(vt_model* m, const float* feat_dev, int32_t B, void* stream, const vt_outputs* out) {
    int rc = check_ready(m, B);
    if (rc) return rc;
    if (!feat_dev) return fail(VT_ERR_ARG, "null device pointer");
    if (m->vb) return run_head_vitb(m, feat_dev, B, static_cast<hipStream_t>(stream), out);
    return run_head(m, feat_dev, B, static_cast<hipStream_t>(stream), out);
}

int vt_forward(vt_model* m, const float* z_dev, const float* x_dev, int32_t B, void* stream, const vt_outputs* out) {
    int rc = check_ready(m, B);
    if (rc) return rc;
    if (!x_dev) return fail(VT_ERR_ARG, "null device pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!z_dev && (rc = check_template_cache(m, B, "vt_forward", !m->vb))) return rc;      // cached template (vt_set_template)
    if (m->vb) return vitb_network(m, z_dev ? vb::Z_GIVEN : vb::Z_CACHED, z_dev, x_dev, nullptr, 0, B, B, 0, st, out, nullptr);
    return vt48_network(m, z_dev, x_dev, false, 0, B, st, out);
}

int vt_set_template(vt_model* m, const float* z_dev, int32_t B, void* stream) {
    int rc = check_ready(m, B);
    if (rc) return rc;
    if (!z_dev) return fail(VT_ERR_ARG, "null device pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    m->tmpl_frames = 0;
    if (m->vb) {      // ViT-Base caches the templates' patch-GEMM operand rows (vitb.hip): cached and uncached steps run the same two GEMMs
        std::string err;
        if ((rc = vb::set_template(m->vb, z_dev, B, nullptr, st, &err))) return fail(rc, err);
    } else if ((rc = vt48_template_rows(m, z_dev, B, st, m->tokens_c.p))) {      // the rows stay in the cached step's own token matrix
        return rc;
    }
    m->tmpl_frames = B;
    m->tmpl_form_batch = m->form_batch;
    return VT_OK;
}

int vt_set_template_slots(vt_model* m, const float* z_dev, const int32_t* slots, int32_t n, void* stream) {
    if (!m) return fail(VT_ERR_ARG, "null model");
    if (int rcc = check_template_cache(m, 1, "vt_set_template_slots", true)) return rcc;
    if (!z_dev || !slots || n < 1 || n > m->tmpl_frames) return fail(VT_ERR_ARG, "vt_set_template_slots: null pointer or n outside [1, cached frames]");
    std::vector<char> seen((size_t)m->tmpl_frames, 0);
    for (int i = 0; i < n; ++i) {
        if (slots[i] < 0 || slots[i] >= m->tmpl_frames)
            return fail(VT_ERR_ARG, "vt_set_template_slots: slot " + std::to_string(slots[i]) + " outside [0, " + std::to_string(m->tmpl_frames) + ")");
        if (seen[(size_t)slots[i]]++) return fail(VT_ERR_ARG, "vt_set_template_slots: slot " + std::to_string(slots[i]) + " named twice");
    }
    int rc = check_ready(m, n);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (m->vb) {
        std::string err;
        rc = vb::set_template(m->vb, z_dev, n, slots, st, &err);
        return rc ? fail(rc, err) : VT_OK;
    }
    if (!m->generic && !m->zstage.p && (rc = m->zstage.alloc(m->zcache.n))) return rc;
    // Stage: stem(z) + block 0's cache rows of the n templates as frames 0..n-1 of the uncached token matrix and of zstage, under the
    // forms vt_set_template picked for the whole cache (by max(form batch, cached frames), not by n).  Every stage is per frame under a
    // given form, so frame i's rows are what the cache holds for that template at any slot.
    {
        struct Restore {      // the form batch and the cache's address, back on every path
            vt_model* m;
            int fb;
            float* zc;
            ~Restore() { m->form_batch = fb; m->zcache.p = zc; }
        } restore{m, m->form_batch, m->zcache.p};
        m->form_batch = std::max(m->tmpl_form_batch, m->tmpl_frames);
        if (!m->generic) m->zcache.p = m->zstage.p;
        if ((rc = vt48_template_rows(m, z_dev, n, st, m->tokens.p))) return rc;
    }
    // ... then into place: each slot's template token rows (rows [0, len_z) of its frame) and its cache rows
    const size_t C = (size_t)m->cfg.channels, trow = (size_t)m->L * C, tz = (size_t)m->len_z * C;
    const size_t zf = m->generic ? 0 : m->zcache.n / (size_t)m->cfg.max_batch;
    for (int i = 0; i < n; ++i) {
        const size_t s = (size_t)slots[i];
        HIP_TRY(hipMemcpyAsync(m->tokens_c.p + s * trow, m->tokens.p + (size_t)i * trow, tz * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (zf) HIP_TRY(hipMemcpyAsync(m->zcache.p + s * zf, m->zstage.p + (size_t)i * zf, zf * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    return VT_OK;
}

int vt_cal_bbox(vt_model* m, const float* score_dev, const float* size_dev, const float* offset_dev, int32_t B,
                void* stream, float* bbox_dev, float* max_score_dev) {
    if (!m || !score_dev || !size_dev || !offset_dev || !bbox_dev || B < 1) return fail(VT_ERR_ARG, "bad argument");
    return run_decode(m, static_cast<hipStream_t>(stream), score_dev, size_dev, offset_dev, nullptr, B, bbox_dev, nullptr,
                      max_score_dev);
}

int vt_crop(vt_model* m, const uint8_t* frames_dev, int32_t H, int32_t W, const double* states_dev, double factor,
            int32_t out_size, const float* mean3, const float* std3, int32_t B, void* stream, float* crops_dev,
            double* resize_factor_dev) {
    return run_crop(m, CropSrc{frames_dev, H, W}, states_dev, factor, out_size, mean3, std3, B, stream, crops_dev, resize_factor_dev, false);
}

int vt_crop_u8(vt_model* m, const uint8_t* frames_dev, int32_t H, int32_t W, const double* states_dev, double factor,
               int32_t out_size, int32_t B, void* stream, uint8_t* patch_dev, double* resize_factor_dev) {
    return run_crop(m, CropSrc{frames_dev, H, W}, states_dev, factor, out_size, nullptr, nullptr, B, stream, patch_dev, resize_factor_dev, true);
}

int vt_crop_frames(vt_model* m, const vt_frame* frames_dev, const double* states_dev, double factor, int32_t out_size,
                   const float* mean3, const float* std3, int32_t B, void* stream, float* crops_dev, double* resize_factor_dev) {
    return run_crop(m, CropSrc{nullptr, 0, 0, frames_dev}, states_dev, factor, out_size, mean3, std3, B, stream, crops_dev, resize_factor_dev, false);
}

int vt_crop_u8_frames(vt_model* m, const vt_frame* frames_dev, const double* states_dev, double factor, int32_t out_size, int32_t B,
                      void* stream, uint8_t* patch_dev, double* resize_factor_dev) {
    return run_crop(m, CropSrc{nullptr, 0, 0, frames_dev}, states_dev, factor, out_size, nullptr, nullptr, B, stream, patch_dev, resize_factor_dev, true);
}

int vt_crop_images(vt_model* m, const vt_image* images_dev, const double* states_dev, double factor, int32_t out_size,
                   const float* mean3, const float* std3, int32_t B, void* stream, float* crops_dev, double* resize_factor_dev) {
    return run_crop(m, CropSrc{nullptr, 0, 0, nullptr, images_dev}, states_dev, factor, out_size, mean3, std3, B, stream, crops_dev, resize_factor_dev, false);
}

int vt_crop_u8_images(vt_model* m, const vt_image* images_dev, const double* states_dev, double factor, int32_t out_size, int32_t B,
                      void* stream, uint8_t* patch_dev, double* resize_factor_dev) {
    return run_crop(m, CropSrc{nullptr, 0, 0, nullptr, images_dev}, states_dev, factor, out_size, nullptr, nullptr, B, stream, patch_dev, resize_factor_dev,
                    true);
}

// Does (mean3, std3) equal the normalisation folded into the uint8 form of layer 1?
static bool same_norm(const vt_model* m, const float* mean3, const float* std3) {
    return std::memcmp(mean3, m->norm_mean, 12) == 0 && std::memcmp(std3, m->norm_std, 12) == 0;
}

int vt_set_normalization(vt_model* m, const float* mean3, const float* std3) {
    if (!m || !mean3 || !std3) return fail(VT_ERR_ARG, "null argument");
    for (int c = 0; c < 3; ++c)
        if (!(std3[c] > 0.f) || !std::isfinite(mean3[c]) || !std::isfinite(std3[c])) return fail(VT_ERR_ARG, "bad mean / std");
    if (same_norm(m, mean3, std3)) return VT_OK;      // already folded (or remembered for vt_load_weights): nothing to replace, no synchronisation
    if (m->graphs_captured > 0) return fail(VT_ERR_STATE, "captured graphs read the folded layer-1 weights: set the normalisation before capturing");
    if (m->vb && !m->weights_loaded) {
        std::string err;
        if (int rc = vb::set_normalization(m->vb, mean3, std3, &err)) return fail(rc, err);
    }
    if (!m->weights_loaded || m->generic) {      // remembered: vt_load_weights folds with these; the shape-generic stem takes them as kernel arguments (not in captured graphs: see above)
        std::memcpy(m->norm_mean, mean3, 12);
        std::memcpy(m->norm_std, std3, 12);
        return VT_OK;
    }
    HIP_TRY(hipDeviceSynchronize());      // no step may be reading the image that is about to be replaced
    if (m->vb) {
        std::string err;
        if (int rc = vb::set_normalization(m->vb, mean3, std3, &err)) return fail(rc, err);
        std::memcpy(m->norm_mean, mean3, 12);
        std::memcpy(m->norm_std, std3, 12);
        return VT_OK;
    }
    return fold_w1u(m, mean3, std3);
}

int vt_set_candidate_elimination(vt_model* m, int32_t n, const int32_t* loc, const double* keep_ratio, const uint8_t* template_rows) {
    std::string err;
    if (int rc = vb::check_ce_args(n, loc, keep_ratio, &err)) return fail(rc, err);      // what needs no model comes first
    if (!m) return fail(VT_ERR_ARG, "null model");
    if (!m->vb) return fail(VT_ERR_ARG, "candidate elimination is implemented for ViT-Base models (channels 768) only");
    if (m->graphs_captured > 0)
        return fail(VT_ERR_STATE, "captured graphs hold the routes and stage buffers of their capture: set the candidate elimination before capturing");
    if (int rc = vb::set_candidate_elimination(m->vb, n, loc, keep_ratio, template_rows, &err)) return fail(rc, err);
    return VT_OK;
}

int vt_set_ce_form(vt_model* m, int32_t form) {
    if (!m) return fail(VT_ERR_ARG, "null model");
    if (!m->vb) return fail(VT_ERR_ARG, "candidate elimination is implemented for ViT-Base models (channels 768) only");
    if (m->graphs_captured > 0)
        return fail(VT_ERR_STATE, "captured graphs hold the routes and stage buffers of their capture: set the candidate-elimination form before capturing");
    std::string err;
    if (int rc = vb::set_ce_form(m->vb, form, &err)) return fail(rc, err);
    return VT_OK;
}

int vt_ce_result(vt_model* m, int32_t B, void* stream, uint8_t* removed_stage_dev, float* scores_dev) {
    if (!m) return fail(VT_ERR_ARG, "null model");
    if (!m->vb) return fail(VT_ERR_ARG, "candidate elimination is implemented for ViT-Base models (channels 768) only");
    std::string err;
    if (int rc = vb::ce_result(m->vb, B, static_cast<hipStream_t>(stream), removed_stage_dev, scores_dev, &err)) return fail(rc, err);
    return VT_OK;
}

int vt_patch_u8_supported(const vt_model* m, int32_t B) {
    if (!m) return 0;
    return stem_takes_u8(m, B) ? 1 : 0;
}

int vt_set_open_loop(vt_model* m, int32_t on) {
    if (!m) return fail(VT_ERR_ARG, "null model");
    m->open_loop = on ? 1 : 0;
    return VT_OK;
}

int vt_gemm_form(const vt_model* m, int32_t B) {
    if (!m) return (void)fail(VT_ERR_ARG, "null model"), -1;
    return m->vb ? vb::gemm_form(m->vb, B) : 0;
}

static const char* const PRECISION_MODELS =
    "the fp32-equivalent mode is implemented for the patch-16 ViT models: vt_create_vit, or the ViT-Base (768, 12) / ViT-Large (1024, 16) tuples of vt_create";

int vt_set_precision(vt_model* m, int32_t precision) {
    if (!m) return fail(VT_ERR_ARG, "null model");
    if (!m->vb) return fail(VT_ERR_ARG, PRECISION_MODELS);
    if (m->graphs_captured > 0)
        return fail(VT_ERR_STATE, "captured graphs hold the routes and workspaces of their capture: set the precision before capturing");
    std::string err;
    const int before = vb::precision(m->vb);
    if (int rc = vb::set_precision(m->vb, precision, &err)) return fail(rc, err);
    if (before != precision) m->tmpl_frames = 0;      // the template cache holds the other mode's operand rows
    return VT_OK;
}

int vt_precision(const vt_model* m) {
    if (!m) return (void)fail(VT_ERR_ARG, "null model"), -1;
    if (!m->vb) return -1;      // a query: another model family has no mode, and asking is no error
    return vb::precision(m->vb);
}

int vt_crop_form(void) {
    bool bytes = false;
    if (crop_selftest(&bytes)) return -1;
    return bytes ? 2 : 1;
}

// the kernels load a patch's 12-byte pixel groups through 4-byte-aligned pointers (ViT-Base: 16-byte rows, checked in vitb.hip)
static int check_patch(const vt_model* m, const void* patch) {
    if (!patch) return fail(VT_ERR_ARG, "null device pointer");
    const uintptr_t mask = m->vb ? 15 : 3;
    if (reinterpret_cast<uintptr_t>(patch) & mask)
        return fail(VT_ERR_ARG, m->vb ? "the uint8 patch must be 16-byte aligned on the ViT-Base path" : "the uint8 patch must be 4-byte aligned");
    return VT_OK;
}

int vt_stem_u8(vt_model* m, const uint8_t* x_patch_dev, int32_t B, void* stream, float* tokens_dev) {
    int rc = check_ready(m, B);
    if (rc || (rc = check_patch(m, x_patch_dev))) return rc;
    if (!tokens_dev) return fail(VT_ERR_ARG, "null device pointer");
    if (m->vb) {
        std::string err;
        rc = vb::stem_rows(m->vb, vb::Z_NONE, nullptr, nullptr, x_patch_dev, B, static_cast<hipStream_t>(stream), tokens_dev, &err);
        return rc ? fail(rc, err) : VT_OK;
    }
    return run_stem(m, nullptr, reinterpret_cast<const float*>(x_patch_dev), B, static_cast<hipStream_t>(stream), tokens_dev, 0, 1, true);
}

int vt_forward_u8(vt_model* m, const float* z_dev, const uint8_t* x_patch_dev, int32_t B, void* stream, const vt_outputs* out) {
    int rc = check_ready(m, B);
    if (rc || (rc = check_patch(m, x_patch_dev))) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!z_dev && (rc = check_template_cache(m, B, "vt_forward_u8", !m->vb))) return rc;      // cached template: the tracker step's network part
    if (m->vb)      // two chains from 64 frames up, as the tracker step
        return vitb_network_chains(m, chain_count(m, B), z_dev ? vb::Z_GIVEN : vb::Z_CACHED, z_dev, nullptr, x_patch_dev, B, st, out, nullptr);
    return vt48_network(m, z_dev, reinterpret_cast<const float*>(x_patch_dev), true, 0, B, st, out);
}

int vt_update_state(vt_model* m, const float* hann_boxes_dev, const double* resize_factor_dev, int32_t search_size,
                    int32_t H, int32_t W, int32_t margin, int32_t B, void* stream, double* states_dev) {
    if (!m || !hann_boxes_dev || !resize_factor_dev || !states_dev || B < 1) return fail(VT_ERR_ARG, "bad argument");
    hipLaunchKernelGGL(vtt::update_state_kernel, dim3((B + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream),
                       hann_boxes_dev, resize_factor_dev, search_size, H, W, margin, B, states_dev, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    return VT_OK;
}

int vt_update_state_record(vt_model* m, const float* hann_boxes_dev, const float* conf_dev, const double* resize_factor_dev,
                           int32_t search_size, int32_t H, int32_t W, int32_t margin, int32_t B, void* stream, double* states_dev,
                           double* record) {
    if (!m || !hann_boxes_dev || !resize_factor_dev || !states_dev || !record || B < 1) return fail(VT_ERR_ARG, "bad argument");
    hipLaunchKernelGGL(vtt::update_state_kernel, dim3((B + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream),
                       hann_boxes_dev, resize_factor_dev, search_size, H, W, margin, B, states_dev, conf_dev, record);
    HIP_TRY(hipGetLastError());
    return VT_OK;
}

// vt_track_step (src.frames: (B,H,W,3)), vt_track_step_frames (src.table: a (B,) vt_frame table) and vt_track_step_images (src.images: a
// (B,) vt_image table; its crop writes the descriptors' sizes into m->imsizes for the tail)
static int track_step(vt_model* m, CropSrc src, double* states_dev, double factor, const float* mean3, const float* std3, int32_t B, void* stream,
                      float* crops_dev, double* resize_factor_dev, const vt_outputs* out, int32_t margin, double* record) {
    int rc = check_ready(m, B);
    if (rc || (rc = check_template_cache(m, B, "vt_track_step", true))) return rc;
    if (!states_dev || !mean3 || !std3 || !crops_dev) return fail(VT_ERR_ARG, "null argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    // The crop reaches the stem as the uint8 patch sample_target returns (a quarter of the fp32 crop's bytes, written and read once)
    // whenever the stem form of this batch reads patches and (mean3, std3) is the normalisation folded into its layer 1; else as the
    // fp32 crop of vt_crop.  Either way crops_dev is the workspace: the patch occupies its first B * S * S * 3 bytes.
    const bool u8 = m->sw.track_u8 != 0 && stem_takes_u8(m, B) && same_norm(m, mean3, std3);
    if (m->vb && u8 && (reinterpret_cast<uintptr_t>(crops_dev) & 15)) return fail(VT_ERR_ARG, "the crop workspace must be 16-byte aligned on the ViT-Base path");
    if (src.images) src.sizes = reinterpret_cast<vt_frame*>(m->imsizes.p);
    if ((rc = run_crop(m, src, states_dev, factor, m->cfg.search_size, mean3, std3, B, stream, crops_dev, resize_factor_dev, u8))) return rc;
    TrackTail tail{resize_factor_dev, states_dev, record, m->cfg.search_size, src.H, src.W, margin, m->open_loop};
    tail.frames = src.images ? src.sizes : src.table;      // the tail clips each sequence against its own frame
    if (m->vb)      // crop on `st`, then the network and each slice's tail on the chains (two from 64 frames up), joined back into `st`
        return vitb_network_chains(m, chain_count(m, B), vb::Z_CACHED, nullptr, u8 ? nullptr : crops_dev,
                                   u8 ? reinterpret_cast<const unsigned char*>(crops_dev) : nullptr, B, st, out, &tail);
    return vt48_network(m, nullptr, crops_dev, u8, 0, B, st, out, &tail);
}

int vt_track_step(vt_model* m, const uint8_t* frames, int32_t H, int32_t W, double* states_dev, double factor, const float* mean3,
                  const float* std3, int32_t B, void* stream, float* crops_dev, double* resize_factor_dev, const vt_outputs* out,
                  int32_t margin, double* record) {
    return track_step(m, CropSrc{frames, H, W}, states_dev, factor, mean3, std3, B, stream, crops_dev, resize_factor_dev, out, margin, record);
}

int vt_track_step_frames(vt_model* m, const vt_frame* frames_dev, double* states_dev, double factor, const float* mean3,
                         const float* std3, int32_t B, void* stream, float* crops_dev, double* resize_factor_dev, const vt_outputs* out,
                         int32_t margin, double* record) {
    if (!frames_dev) return fail(VT_ERR_ARG, "null argument");
    return track_step(m, CropSrc{nullptr, 0, 0, frames_dev}, states_dev, factor, mean3, std3, B, stream, crops_dev, resize_factor_dev, out, margin, record);
}

int vt_track_step_images(vt_model* m, const vt_image* images_dev, double* states_dev, double factor, const float* mean3,
                         const float* std3, int32_t B, void* stream, float* crops_dev, double* resize_factor_dev, const vt_outputs* out,
                         int32_t margin, double* record) {
    if (!images_dev) return fail(VT_ERR_ARG, "null argument");
    return track_step(m, CropSrc{nullptr, 0, 0, nullptr, images_dev}, states_dev, factor, mean3, std3, B, stream, crops_dev, resize_factor_dev, out, margin,
                      record);
}

int vt_graph_capture_steps(vt_model* m, int32_t nsteps, const float* const* z_dev, const float* const* x_dev, int32_t B,
                           const vt_outputs* out, vt_graph** g) {
    int rc = check_ready(m, B);
    if (rc) return rc;
    if (!g) return fail(VT_ERR_ARG, "null graph out");
    if (nsteps < 1 || nsteps > 64 || !x_dev) return fail(VT_ERR_ARG, "vt_graph_capture_steps: 1..64 steps, x_dev must not be null");
    // One step may be captured as NCH independent chains over frame slices (fork_join): the kernels of one slice can then overlap
    // the kernels of the others.  Measured slower with the one-workgroup-per-frame kernels (large LDS: no two workgroups share
    // a CU): 107.7 -> 132 us with 2 chains -- so vit_48 defaults to one chain; ViT-Base: two from 64 frames up (read_switches).
    // Several steps, the vit_48 template cache (not sliced) and the shape-generic kernels (ONE set of scratch buffers g_a, g_b, g_x, ...:
    // concurrent chains would race on them) are captured as one chain.
    const bool cached = !z_dev || !z_dev[0];
    const int nch = (nsteps > 1 || (cached && !m->vb) || m->generic) ? 1 : chain_count(m, B);
    if (cached && nch > 1 && (rc = check_template_cache(m, B, "vt_graph_capture", false))) return rc;
    vt_graph* vg = new vt_graph();
    hipError_t e = hipStreamBeginCapture(m->cap_stream, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) { delete vg; return fail(VT_ERR_HIP, std::string("hipStreamBeginCapture: ") + hipGetErrorString(e)); }
    if (nch == 1) {
        for (int i = 0; i < nsteps && !rc; ++i)
            rc = vt_forward(m, z_dev ? z_dev[i] : nullptr, x_dev[i], B, m->cap_stream, out ? &out[i] : nullptr);
    } else {
        const float* const z = cached ? nullptr : z_dev[0];
        const int cus = m->vb ? chain_cus(m, nch) : 0;      // the chains' persistent GEMMs split the CUs between them
        rc = fork_join(m, m->cap_stream, nch, B, [&](int c, size_t f0, int nb, hipStream_t cs) {
            if (m->sw.chain_delay_us > 0 && c > 0)      // a chain may start late (VT_CHAIN_DELAY_US x chain index), so that identical chains do not run in lock step
                hipLaunchKernelGGL(chain_delay_kernel, dim3(1), dim3(64), 0, cs, (unsigned long long)c * m->sw.chain_delay_us * 100ull);
            if (m->vb) return vitb_network(m, z ? vb::Z_GIVEN : vb::Z_CACHED, z, x_dev[0], nullptr, f0, nb, B, cus, cs, out, nullptr);
            return vt48_network(m, z, x_dev[0], false, f0, nb, cs, out);
        });
    }
    e = hipStreamEndCapture(m->cap_stream, &vg->graph);
    if (rc) { if (vg->graph) (void)hipGraphDestroy(vg->graph); delete vg; return rc; }
    if (e != hipSuccess) { delete vg; return fail(VT_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e)); }
    e = hipGraphInstantiate(&vg->exec, vg->graph, nullptr, nullptr, 0);
    if (e != hipSuccess) { (void)hipGraphDestroy(vg->graph); delete vg; return fail(VT_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e)); }
    vg->owner = m;
    m->graphs.push_back(vg);
    *g = vg;
    ++m->graphs_captured;
    return VT_OK;
}

int vt_graph_capture(vt_model* m, const float* z_dev, const float* x_dev, int32_t B, const vt_outputs* out, vt_graph** g) {
    return vt_graph_capture_steps(m, 1, &z_dev, &x_dev, B, out, g);
}

int vt_graph_launch(vt_graph* g, void* stream) {
    if (!g || !g->exec) return fail(VT_ERR_ARG, "null graph");
    if (!g->owner) return fail(VT_ERR_STATE, "vt_graph_launch: the graph's model was destroyed (its kernels would run on freed workspaces)");
    HIP_TRY(hipGraphLaunch(g->exec, static_cast<hipStream_t>(stream)));
    return VT_OK;
}

void vt_graph_destroy(vt_graph* g) {
    if (!g) return;
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    if (g->graph) (void)hipGraphDestroy(g->graph);
    if (g->owner) {      // the last graph gone: vt_set_form_batch / vt_set_normalization are free again
        auto& v = g->owner->graphs;
        v.erase(std::remove(v.begin(), v.end(), g), v.end());
        if (g->owner->graphs_captured > 0) --g->owner->graphs_captured;
    }
    delete g;
}

int vt_debug_stamps(vt_model* m, int32_t B, unsigned long long* host_out) {
    // Development aid: copies the in-kernel s_memtime stamps of the last launch (block kernel: [B][waves][64];
    // stem_fused / stem_pipe: [B][16][32]); the buffer holds B * 8 * 64 values.
    if (!m || !m->dbg_stamps || !host_out) return fail(VT_ERR_STATE, "stamps are off (set VT_DBG_STAMPS=1 before vt_create)");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host_out, m->dbg_stamps, (size_t)B * 8 * 64 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return VT_OK;
}

int vt_probe_clock(int32_t iters, int32_t waves_per_simd, double* mhz, double* cycles_per_mfma, double* wall_us) {
    // Development probe (not on the hot path; synchronises): sustained shader clock under a dense
    // f32-MFMA loop and the cycles one SIMD spends per v_mfma_f32_16x16x4_f32.
    if (iters < 1 || waves_per_simd < 1 || waves_per_simd > 4) return fail(VT_ERR_ARG, "bad probe arguments");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, 0));
    const int nwg = prop.multiProcessorCount * waves_per_simd;
    float *src = nullptr, *sink = nullptr;
    unsigned long long* st = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&src), 512 * sizeof(float)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&sink), (size_t)nwg * 256 * sizeof(float)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&st), (size_t)nwg * 8 * sizeof(unsigned long long)));
    std::vector<float> h(512);
    for (int i = 0; i < 512; ++i) h[i] = 0.25f + 0.001f * (float)((i * 37) % 101);
    HIP_TRY(hipMemcpy(src, h.data(), 512 * sizeof(float), hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    hipLaunchKernelGGL(probe_kernel, dim3(nwg), dim3(256), 0, nullptr, src, iters, st, sink);   // warm-up
    HIP_TRY(hipEventRecord(e0, nullptr));
    hipLaunchKernelGGL(probe_kernel, dim3(nwg), dim3(256), 0, nullptr, src, iters, st, sink);
    HIP_TRY(hipEventRecord(e1, nullptr));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    std::vector<unsigned long long> hs((size_t)nwg * 8);
    HIP_TRY(hipMemcpy(hs.data(), st, hs.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    std::vector<double> f, c;
    for (size_t k = 0; k < hs.size(); k += 2) {
        f.push_back((double)hs[k] / (double)hs[k + 1] * 100.0);
        c.push_back((double)hs[k] / ((double)iters * 8.0) / waves_per_simd);
    }
    std::sort(f.begin(), f.end());
    std::sort(c.begin(), c.end());
    if (mhz) *mhz = f[f.size() / 2];
    if (cycles_per_mfma) *cycles_per_mfma = c[c.size() / 2];
    if (wall_us) *wall_us = ms * 1e3;
    (void)hipFree(src); (void)hipFree(sink); (void)hipFree(st);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return VT_OK;
}

int vt_selftest_mfma(void* stream) {
    // exact small integers; B is asymmetric so a transposed read or write cannot pass
    std::vector<float> A(256), Bm(256), D(384, -1.f), ref(256, 0.f);
    for (int i = 0; i < 16; ++i)
        for (int k = 0; k < 16; ++k) {
            A[i * 16 + k] = (float)((i * 3 + k * 5) % 7 - 3);
            Bm[i * 16 + k] = (float)((i * 11 + k * 2) % 9 - 4);   // B[k=i][j=k]
        }
    for (int i = 0; i < 16; ++i)
        for (int j = 0; j < 16; ++j)
            for (int k = 0; k < 16; ++k) ref[i * 16 + j] += A[i * 16 + k] * Bm[k * 16 + j];
    float *dA = nullptr, *dB = nullptr, *dD = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&dA), 1024));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&dB), 1024));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&dD), 1536));
    HIP_TRY(hipMemcpy(dA, A.data(), 1024, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dB, Bm.data(), 1024, hipMemcpyHostToDevice));
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(mfma_selftest_kernel, dim3(1), dim3(64), 0, st, dA, dB, dD);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(D.data(), dD, 1536, hipMemcpyDeviceToHost));
    (void)hipFree(dA); (void)hipFree(dB); (void)hipFree(dD);
    int bad = 0;
    for (int i = 0; i < 256; ++i) bad += (D[i] != ref[i]);
    if (bad) return fail(VT_ERR_STATE, "MFMA lane map differs from the assumed one in " + std::to_string(bad) + " / 256 elements");
    for (int l = 0; l < 64; ++l) bad += (D[256 + l] != 15.f * ((l & 15) + 1)) + (D[320 + l] != 8.f * ((l & 15) + 1));
    if (bad) return fail(VT_ERR_STATE, "v_permlane16/32_swap lane map differs from the assumed one (" + std::to_string(bad) + " / 128)");
    return VT_OK;
}

}  // extern "C"

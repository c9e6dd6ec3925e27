// vitb.hip -- host side of the plain-ViT OSTrack path (ViT-Base, BASELINE config 4, and ViT-Large): weight packing (bf16, BatchNorm folded, conv
// weights as [cout][tap][cin], attention scale folded into W_q), workspace, launch sequence.  Kernels: vb_gemm.h, vb_misc.h and the
// three attention kernels vb_attn.h, vb_qkvattn.h, vb_attn_stream.h (the 384 geometry's), whose shared arithmetic lives in vb_attn.h;
// vb_ce.h: OSTrack candidate elimination by key masking or compacted (the stages' score / select / gather kernels; vb::blocks routes them).
// vb_f32.h: the fp32-equivalent mode (vb::set_precision): the same GEMM kernel on operands expanded to six bf16 k-ranges, f32 activations, f32
// attention and head tail; blocks_f32 / head_f32 below are its routes (the stem shares run_stem_rows with the bf16 mode: StemRoute holds what
// differs), ModeF32 its workspaces and weight images, for_chunks its launches below the GEMMs' 32-bit operand offsets.
// Reached through the same C ABI as the vit_48 path (vt_create with channels = 768, or the ViT-Large tuple at channels = 1024; vt_create_vit for
// those two and for ViT-Small 384 / 6 and ViT-Tiny 192 / 3).  The model points differ in width, head count and hidden width alone (VbModel::C /
// HEADS / HID, a row of POINTS); the kernels take them at run time except the three that compile the width in (dispatch_width below).  What the two small
// widths need beyond that: launch_wide (an odd number of k-tiles), tile_pad (N no multiple of 256), patch_operand (rows shorter than 768).
// Layout of this file: Buf owns device memory (a model is freed by deleting it); Hooks holds the experiment switches, read once;
// SliceView holds what a frame slice addresses, built once per entry; run_attention launches one of the four attention forms;
// alloc_workspaces allocates a model's (or the fp32 mode's) workspaces, all or none.
#include "vb_api.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vb_attn.h"
#include "vb_attn_stream.h"
#include "vb_ce.h"
#include "vb_f32.h"
#include "vb_gemm.h"
#include "vb_misc.h"
#include "vb_qkvattn.h"

using vbg::bf16;

namespace {

constexpr int HD = 64, PATCH_K = 768, HW = 256 /* head width */;
// The model points: width, heads of 64 (the MLP width is 4 x width), the deepest model admitted, the heads the fused qkv + attention kernel
// walks together, and the name the refusals use.  ViT-Base / ViT-Large: lib/models/ostrack/vit.py:393-400, the two vt_create knows.  The
// small patch-16 students (build_small_ostrack, lib/models/ostrack/ostrack.py:288-342; timm's DeiT-Small / DeiT-Tiny): vb::create_vit only.
// hgroup: 6 of 12 heads measured best at width 768 (vb_qkvattn.h); 16 heads of width 1024 take 4, the divisor whose group of weight rows
// (4 x 384 KiB) is nearest to that one's (6 x 288 KiB); ViT-Small / ViT-Tiny all 6 / 3 heads of a frame together -- their whole qkv matrix,
// 864 / 216 KiB, is smaller than one such group.  max_depth is what the refusals check, and vt_create's ViT-Base tuple is refused by no
// depth of its own (vb::create): that row's 24 is what build_model admits for any model.
struct ModelPoint {
    int C, heads, max_depth, hgroup;
    bool vt_create;
    const char* name;
};
constexpr ModelPoint POINTS[] = {{768, 12, 24, 6, true, "ViT-Base"}, {1024, 16, 24, 4, true, "ViT-Large"}, {384, 6, 12, 6, false, "ViT"}, {192, 3, 12, 3, false, "ViT"}};
constexpr int NPOINTS = sizeof(POINTS) / sizeof(POINTS[0]);
constexpr int C_BASE = POINTS[0].C, C_LARGE = POINTS[1].C, C_SMALL = POINTS[2].C, C_TINY = POINTS[3].C;      // (names for the kernel lists below)
const ModelPoint* model_point(int C) {
    for (const ModelPoint& p : POINTS)
        if (p.C == C) return &p;
    return nullptr;
}
// The two geometries (template / search crop -> tokens at stride 16): OSTrack-256 = 128 / 256 -> 64 + 256 = 320, OSTrack-384 = 192 / 384 ->
// 144 + 576 = 720.  The model carries its own (VbModel::L, LZ, LX, F, TZ, TX); the token counts below are the attention kernels' template arguments.
constexpr int L256 = 320, L384 = 720;
constexpr float LN_EPS = 1e-6f;
// The automatic tile choice (narrow_pick): narrow where the 256 x 256 tiles of a launch number at most this many per cent of the slice's CUs
// (the sweep of tools/vitb_latency.py)
constexpr int NARROW_FILL = 33;
constexpr int HEAD_CH[5] = {0 /* the model's width: VbModel::head_ch */, 256, 128, 64, 32};
// Weight rows per tower of the head's conv li + 1 (cout output channels).  conv1: towers along N (K = 9 x the model's width), no padding.
// conv2 (N = 128 per tower, K = 2304) runs on the 256 x 256 software-pipelined tile, one group per tower, with its weight rows zero-padded
// to 256 (half of every MFMA column block is padding, and it still beats the two-buffer 256 x 64 loop: 268 -> ~180 us, round 5); conv3 /
// conv4 keep the narrow tile (BN = 64: rows padded to 64)
constexpr int head_rows(int li, int cout) { return li == 0 ? cout : (li == 1 ? 256 : (cout < 64 ? 64 : cout)); }

struct Err {
    std::string* e;
    int fail(int code, const std::string& msg) const { if (e) *e = msg; return code; }
};

#define VB_HIP(expr)                                                                                          \
    do {                                                                                                      \
        hipError_t _e = (expr);                                                                               \
        if (_e != hipSuccess) return E.fail(VT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));   \
    } while (0)

uint16_t f2bf(float f) {   // round to nearest even, NaN kept quiet
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

template <typename T>
struct Buf {      // owns its device memory; movable (std::vector<BlockW> is resized), not copyable
    T* p = nullptr;
    size_t n = 0;
    Buf() = default;
    Buf(Buf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; }
    Buf& operator=(Buf&& o) noexcept { std::swap(p, o.p); std::swap(n, o.n); return *this; }
    ~Buf() { release(); }
    hipError_t alloc(size_t count) { n = count; return hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T)); }
    void release() { if (p) (void)hipFree(p); p = nullptr; }
};

// One workspace of a list (alloc_workspaces): a Buf of any element type, its element count, whether it starts zero-filled
struct WsBuf {
    void** p;
    size_t* n;
    size_t count, elem;
    bool zero;
    template <typename T>
    WsBuf(Buf<T>& b, size_t count, bool zero = false) : p(reinterpret_cast<void**>(&b.p)), n(&b.n), count(count), elem(sizeof(T)), zero(zero) {}
};
struct KernelLds { const void* kernel; int lds; };      // a kernel and the dynamic LDS it is launched with
template <typename K>
const void* kernel_ptr(K kernel) { return reinterpret_cast<const void*>(kernel); }

// Allocates every workspace of the list, zero-fills the marked ones and raises the kernels' dynamic LDS limit.  All or none: the first
// error is returned, with every buffer of the list released.  *bytes (optional): the bytes asked for.
hipError_t alloc_workspaces(std::initializer_list<WsBuf> bufs, std::initializer_list<KernelLds> kernels, size_t* bytes = nullptr) {
    hipError_t e = hipSuccess;
    for (const WsBuf& w : bufs) {
        if (bytes) *bytes += w.count * w.elem;
        if (e == hipSuccess) {
            *w.n = w.count;
            e = hipMalloc(w.p, w.count * w.elem);
        }
    }
    for (const WsBuf& w : bufs)
        if (w.zero && e == hipSuccess) e = hipMemset(*w.p, 0, w.count * w.elem);
    for (const KernelLds& k : kernels)
        if (e == hipSuccess) e = hipFuncSetAttribute(k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, k.lds);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        for (const WsBuf& w : bufs) {
            if (*w.p) (void)hipFree(*w.p);
            *w.p = nullptr;
        }
    }
    return e;
}

struct BlockW {
    Buf<float> ln1g, ln1b, ln2g, ln2b, bqkv, bproj, b1, b2;
    Buf<bf16> wqkv, wproj, w1, w2;
};

// The fp32-equivalent mode (vb_f32.h).  Per block: the host's unfolded f32 tensors (q rows and bias times the attention scale),
// kept from vt_load_weights so that vt_set_precision can come later, and their expanded piece images [N (padded)][6 K] on the device.
struct BlockF {
    std::vector<float> h_wqkv, h_bqkv, h_wproj, h_w1, h_b1, h_w2;
    Buf<bf16> wqkv, wproj, w1, w2;
    Buf<float> bqkv, b1;
};
// What the mode adds to a model: workspaces (allocated when the mode is first selected) and weight images (built when mode and weights meet)
struct ModeF32 {
    bool ws = false, weights = false;
    Buf<bf16> x6;            // [max rows][6 C]: the LayerNorms' and the attention's output, the operand of qkv / fc1 / proj
    Buf<bf16> hid6;          // [max rows][6 HID]: GELU's output, fc2's operand (and the patch operand of the widths below 768)
    Buf<float> hid32;        // [max rows][HID]: fc1's pre-activation; q | k | v [rows][3 C] of a slice lives in the same rows
    Buf<float> feat32;       // [max_batch][LX][C]: the final norm's search rows
    Buf<float> tmp32;        // [max_batch][LX][768]: a head conv's f32 output, slice by slice
    Buf<bf16> map6[4];       // the head's zero-bordered maps of expanded pixels (map_split_kernel)
    Buf<bf16> zop6;          // template cache: [max_batch * LZ][6 x 768]
    Buf<bf16> wpatch, wpatch_u8, wc[4];
    Buf<float> bpatch_u8;
    std::vector<BlockF> blk;
    std::vector<float> h_wc[4];      // the head's folded conv weights [3 towers][rows][9 cin] as load_weights lays them out
};

}  // namespace

struct VbModel {
    vt_config cfg{};
    int depth = 12, maxB = 0;
    int C = POINTS[0].C, HEADS = POINTS[0].heads, HID = 4 * POINTS[0].C;      // width, heads, MLP width: a row of POINTS
    int head_ch(int i) const { return i ? HEAD_CH[i] : C; }    // channels of the head's map i
    int stat_p() const { return C / 64; }      // (sum, M2) pairs per residual row: one per 64-column wave slice of the 256-wide GEMM tiles
    int TZ = 128, TX = 256, LZ = 64, LX = 256, L = 320, F = 16;      // crop sides, template / search / all tokens per frame, head map side
    int zshift = 6, xshift = 8;     // log2(LZ), log2(LX) where they are powers of two (EPI_PATCH_ROWS); -1 otherwise (EPI_PATCH_ROWS_N)
    bool g384 = false;              // OSTrack-384: always qk GEMM + v GEMM + vbs::attn_stream_kernel (VB_FUSED_QKV has no effect)
    bool attn_stream = false;       // VB_ATTN_STREAM (with VB_FUSED_QKV=0): the streaming attention kernel at the 256 geometry too
    bool loaded = false;
    // parameters
    Buf<bf16> wpatch; Buf<float> bpatch, pos, ng, nb;
    std::vector<BlockW> blk;
    Buf<bf16> wc[4]; Buf<float> bc[4], w5, b5;     // head: conv1 (towers along N), conv2..4 ([3][cout_padded][9 cin])
    // workspace
    Buf<bf16> xn, qk, vt, ao, hid, map[4], t4;      // map[i]: the head's zero-bordered maps of HEAD_CH[i] channels (1-3: three towers)
    Buf<float> resid;
    // LayerNorm folded into qkv / fc1 (vb_gemm.h): xn then holds the RAW residual rows in bf16, written by the GEMM epilogues that
    // produce them, rstd their 1 / sqrt(var + eps), stats the epilogues' per-slice (sum, M2) pairs [stat_p()][max rows]
    bool fold = true;
    bool fused_qkv = true;          // VB_FUSED_QKV: the qkv projection inside the attention kernel (vb_qkvattn.h) instead of qk GEMM + v GEMM + attention
    Buf<float> rstd;
    Buf<float> rmean;        // per-row mean of the residual stream as of the last finalize: the next producer centres its bf16 copy on it
    Buf<float> cpos;         // [L]: mean over channels of (pos-embed row + patch bias): the patch GEMM's centring constant per token
    // uint8 search patches (vb::stem_rows): Preprocessor.process folded into a second image of the patch weights (fold_patch_u8), the
    // centring table rebuilt from its bias; host copies of what the fold starts from, for vt_set_normalization after vt_load_weights
    Buf<bf16> wpatch_u8; Buf<float> bpatch_u8, cpos_u8;
    std::vector<float> h_wpatch, h_bpatch, h_pos;
    float norm_mean[3] = {0.485f, 0.456f, 0.406f}, norm_std[3] = {0.229f, 0.224f, 0.225f};
    float u8_centre = 128.f;        // VB_U8_CENTER=0: the uncentred fold (diagnostic: NOTES R7-1 shows it over the token bound)
    Buf<bf16> zop;           // template cache: the templates' operand rows [max_batch * LZ][PATCH_K]
    bool center = true;      // VB_LN_CENTER
    // VB_GEMM_NARROW (read at vt_create): -1 = per launch, the 128 x 64 tile where the 256 x 256 tiles would fill at most narrow_fill per cent
    // of the slice's CUs (narrow_pick); 0 = never; 1 = wherever a narrow instantiation exists.  Both tiles give the same bits (vb_gemm.h)
    int gemm_narrow = -1;
    int narrow_fill = NARROW_FILL;      // VB_GEMM_NARROW_FILL: the threshold of the automatic choice (tools/vitb_latency.py sweeps it)
    Buf<vbg::f2> stats;
    // candidate elimination by key masking (vb_ce.h; vb::set_candidate_elimination).  ce_loc / ce_keep: per stage its block and its count of
    // kept search tokens (a count equal to the previous one: the stage is a no-op and runs nothing); ce_first: the block of the first stage
    // that removes something, -1 = a plain model.  Device buffers, all indexed by absolute frame: ce_bits [stage][max_batch][ceil(L / 32)] the
    // key bitmap each stage leaves, ce_removed [max_batch][LX], ce_scores [stage][max_batch][LX], ce_part [max_batch][HEADS][LX] the
    // per-head sums between the two kernels of a stage, ce_rows the selected template rows
    std::vector<int> ce_loc, ce_keep;
    int ce_first = -1, ce_nrows = 0;
    bool ce_set = false;
    bool ce_plain = false;          // VB_CE_SCORE_PLAIN=1: the plain score loop for ALL too (the MFMA form's yardstick; tests)
    Buf<uint32_t> ce_bits;
    Buf<uint8_t> ce_removed;
    Buf<float> ce_scores, ce_part;
    Buf<int32_t> ce_rows;
    int ce_words() const { return (L + 31) / 32; }
    // the compact form (vb::set_ce_form, vb_ce.h): behind every stage the kept tokens are gathered into frames of ce_lp(k) rows.  ce_index
    // [stage][max_batch][ce_keep[stage]] (stage k from element ce_index_off[k]): the global search index of every compacted search row;
    // ce_src [max_batch][LX]: per kept token its number among the stage's candidates (select -> gather); ce_inv [max_batch][LX]: the
    // compacted search row of a global token after the last stage that ran, -1 = removed (the final norm's scatter)
    int ce_form = VT_CE_MASKED;
    Buf<int32_t> ce_index, ce_src, ce_inv;
    std::vector<size_t> ce_index_off;
    int ce_lp(int k) const { return (LZ + ce_keep[k] + 15) / 16 * 16; }
    int precision = VT_PRECISION_BF16;      // vb::set_precision
    ModeF32 f32;
};

namespace {

int need(const vb::TensorMap& tm, const std::string& name, int64_t numel, const float** out, const Err& E) {
    auto it = tm.find(name);
    if (it == tm.end()) return E.fail(VT_ERR_MISSING_KEY, "missing key in state dict: " + name);
    if (it->second.second != numel)
        return E.fail(VT_ERR_MISSING_KEY, "shape mismatch for " + name + ": got " + std::to_string(it->second.second) +
                                              " elements, want " + std::to_string(numel));
    *out = it->second.first;
    return VT_OK;
}

// d holds `count` elements afterwards: reallocated if its size was another
template <typename T>
int ensure(Buf<T>& d, size_t count, const Err& E) {
    if (!d.p || d.n != count) {
        d.release();
        VB_HIP(d.alloc(count));
    }
    return VT_OK;
}
template <typename T>
int upload(Buf<T>& d, const void* h, size_t count, const Err& E) {
    if (int rc = ensure(d, count, E)) return rc;
    VB_HIP(hipMemcpy(d.p, h, count * sizeof(T), hipMemcpyHostToDevice));
    return VT_OK;
}

// pad: zero elements behind the tensor (tile_pad)
int upload_bf16(Buf<bf16>& d, const std::vector<float>& h, const Err& E, size_t pad = 0) {
    std::vector<uint16_t> t(h.size() + pad, 0);
    for (size_t i = 0; i < h.size(); ++i) t[i] = f2bf(h[i]);
    return upload(d, t.data(), t.size(), E);
}
// The 256-wide tiles fetch whole 256-row weight panels: a weight matrix whose last GEMM has N rows (N = 192, 384: no multiple of 256) carries
// zero rows up to the end of that GEMM's last column tile.  Nothing computed from them is stored (the epilogues skip wave slices past N).
size_t tile_pad(int N, int K) { return (size_t)((N + 255) / 256 * 256 - N) * K; }
int upload_f32(Buf<float>& d, const float* h, size_t n, const Err& E) { return upload(d, h, n, E); }

// a state-dict tensor as it is: looked up, checked and uploaded, one helper per element type (*host: the tensor's host values)
int load_f32(Buf<float>& d, const vb::TensorMap& tm, const std::string& name, int64_t numel, const Err& E, const float** host = nullptr) {
    const float* p;
    if (int rc = need(tm, name, numel, &p, E)) return rc;
    if (host) *host = p;
    return upload_f32(d, p, (size_t)numel, E);
}
int load_bf16(Buf<bf16>& d, const vb::TensorMap& tm, const std::string& name, int64_t numel, const Err& E, const float** host = nullptr, size_t pad = 0) {
    const float* p;
    if (int rc = need(tm, name, numel, &p, E)) return rc;
    if (host) *host = p;
    return upload_bf16(d, std::vector<float>(p, p + numel), E, pad);
}

int num_cus() {
    static int n = 0;
    if (!n) {
        hipDeviceProp_t prop;
        n = hipGetDeviceProperties(&prop, 0) == hipSuccess ? prop.multiProcessorCount : 256;
    }
    return n;
}

inline int env_int(const char* name, int dflt) { const char* v = std::getenv(name); return v ? std::atoi(v) : dflt; }

// The experiment hooks (tools/gpu_vbdbg.sh, gpu_vbexp.sh, gpu_vbchains.sh), read once, at the first GEMM launch:
//   VB_DBG                              vbg::Args::dbg of every GEMM
//   VB_RB_<epilogue id>=rows            overrides the tile-row block of that GEMM kind
//   VB_DESYNC_<epilogue id>=<us>[:groups]   phase groups of workgroups (Args::desync_ticks)
//   VB_MAX_CUS                          persistent grids of at most this many workgroups
struct Hooks {
    int dbg, max_cus, rb[8], desync_us[8], desync_groups[8];
    Hooks() : dbg(env_int("VB_DBG", 0)), max_cus(env_int("VB_MAX_CUS", 0)) {
        for (int e = 0; e < 8; ++e) {
            rb[e] = env_int(("VB_RB_" + std::to_string(e)).c_str(), -1);
            const char* v = std::getenv(("VB_DESYNC_" + std::to_string(e)).c_str());
            desync_us[e] = v ? std::atoi(v) : 0;
            const char* c = v ? std::strchr(v, ':') : nullptr;
            desync_groups[e] = c ? std::max(2, std::atoi(c + 1)) : 2;
        }
    }
};
const Hooks& hooks() { static const Hooks h; return h; }

// workgroups of a persistent kernel: one per CU, at most `cus` (0 = all), in whole XCD rounds of 8
int persistent_grid(int cus, int groups = 1) { return std::max(8, (cus > 0 ? std::min(cus, num_cus()) : num_cus()) / groups / 8 * 8); }

// grid of a grid-stride elementwise kernel of 256 threads
unsigned grid256(size_t items) { return (unsigned)std::min<size_t>((items + 255) / 256, 16384); }

template <int BM, int BN, int WM, int WN, int AMODE, int EPI>
int launch_gemm(const vbg::Args& a, int groups, hipStream_t st, const Err& E, int cus = 0) {
    if (a.M < 1 || a.K % vbg::BK != 0 || a.N % 8 != 0)
        return E.fail(VT_ERR_ARG, "gemm shape: K must be a multiple of 64 and N of 8 (got M=" + std::to_string(a.M) + " N=" +
                                      std::to_string(a.N) + " K=" + std::to_string(a.K) + ")");
    if (BM == 256 && BN == 256 && !(AMODE & vbg::A_ANYK) && a.K % (2 * vbg::BK) != 0) return E.fail(VT_ERR_ARG, "gemm shape: the 256 x 256 tile needs K to be a multiple of 128");
    const Hooks& H = hooks();
    vbg::Args ad = a;
    ad.dbg = H.dbg;
    if constexpr (EPI < 8) {      // (the hooks know the bf16 mode's eight epilogues)
        if (H.rb[EPI] >= 0) ad.rb = H.rb[EPI];
        if (H.desync_us[EPI] > 0) { ad.desync_ticks = H.desync_us[EPI] * 100; ad.desync_groups = H.desync_groups[EPI]; }
    }
    // persistent workgroups: one per CU, each walks tiles blockIdx.x, blockIdx.x + grid, ...
    const int ntiles = ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN);
    if (H.max_cus > 0) cus = cus > 0 ? std::min(cus, H.max_cus) : H.max_cus;
    const int tiles = std::min(ntiles, persistent_grid(cus, groups));
    constexpr int lds = vbg::lds_bytes<BM, BN>();
    hipLaunchKernelGGL((vbg::gemm_kernel<BM, BN, WM, WN, AMODE, EPI>), dim3(tiles, groups), dim3(512), lds, st, ad);
    VB_HIP(hipGetLastError());
    return VT_OK;
}

// The kernels that compile the width in (vbm::layernorm_kernel<C>, vbm::ln_finalize_kernel<C / 64>, the fused qkv + attention kernel): f
// is called with the model's width as a std::integral_constant: the row of POINTS with that width.  vb::create / vb::create_vit admit no other
// (a width outside the table would run the last row's instantiation).
template <int I = 0, typename F>
void dispatch_width(int C, F&& f) {
    if constexpr (I + 1 < NPOINTS)
        if (C != POINTS[I].C) return dispatch_width<I + 1>(C, f);
    f(std::integral_constant<int, POINTS[I].C>{});
}

// The kernels that compile the frame length in (the streaming attention and the candidate-elimination scores on full frames): f is called
// with the model's tokens per frame, L256 or L384, as a std::integral_constant.
template <typename F>
void dispatch_geo(const VbModel* m, F&& f) {
    if (m->g384) f(std::integral_constant<int, L384>{});
    else f(std::integral_constant<int, L256>{});
}

// Which tile a GEMM launch runs, from its count of 256 x 256 tiles and the slice's CUs alone: the narrow tile where the wide ones would leave
// most of the CUs idle.  One rule for launch_tile and vb::gemm_form.
bool narrow_pick(const VbModel* m, int M, int N, int groups, int cus) {
    if (m->gemm_narrow >= 0) return m->gemm_narrow != 0;
    const long long wide = (long long)((M + 255) / 256) * ((N + 255) / 256) * groups;
    const int budget = cus > 0 ? std::min(cus, num_cus()) : num_cus();
    return wide * 100 <= (long long)m->narrow_fill * budget;
}

// A GEMM kind of the ViT path on the tile narrow_pick chooses for this launch
// The wide form of a GEMM kind.  The 256 x 256 tile's software-pipelined loop takes k-tiles in pairs; an odd count (ViT-Tiny: K = 192 of qkv /
// proj / fc1, K = 9 x 192 of the head's conv1) goes to a tile on the two-buffer loop, which takes any: the same 256 x 256 tile for the
// token GEMMs (A_ANYK), the head's 256 x 64 tile for conv1.  Same k order from zero, same epilogue, same 64-column wave slices: same bits.
template <int AMODE, int EPI>
int launch_wide(const vbg::Args& a, int groups, hipStream_t st, const Err& E, int cus) {
    if (a.K % (2 * vbg::BK) != 0) {
        if constexpr (AMODE == vbg::A_CONV) return launch_gemm<256, 64, 8, 1, vbg::A_CONV, vbg::EPI_CONV>(a, groups, st, E, cus);
        else if constexpr (EPI == vbg::EPI_BF16 || EPI == vbg::EPI_VT || EPI == vbg::EPI_RESID || EPI == vbg::EPI_GELU)
            return launch_gemm<256, 256, 2, 4, AMODE | vbg::A_ANYK, EPI>(a, groups, st, E, cus);
    }
    return launch_gemm<256, 256, 2, 4, AMODE, EPI>(a, groups, st, E, cus);      // (the patch GEMMs: K = 768 at every width)
}

template <int AMODE, int EPI>
int launch_tile(const VbModel* m, const vbg::Args& a, int groups, hipStream_t st, const Err& E, int cus) {
    if (narrow_pick(m, a.M, a.N, groups, cus)) return launch_gemm<128, 64, 8, 1, AMODE, EPI>(a, groups, st, E, cus);
    // (N = 384 / 192 stays on the 256-wide tile, a quarter of whose columns are padding there: proj / fc2 on a tile that fits N -- 256 x 128 /
    // 256 x 64 on the two-buffer loop -- measured SLOWER, 6.94 against 6.42 ms and 3.37 against 3.02 ms per step of 256 frames: NOTES.md)
    return launch_wide<AMODE, EPI>(a, groups, st, E, cus);
}

// rows: the residual rows when they are not B frames of L (the compact form of candidate elimination; then no map / feat)
int run_layernorm(const VbModel* m, const float* resid, const float* g, const float* b, int B, hipStream_t st, bf16* xn, bf16* map, float* feat,
                  const Err& E, bf16* xb = nullptr, float* rstd = nullptr, float* mean = nullptr, int rows = 0) {
    const int M = rows ? rows : B * m->L;
    dispatch_width(m->C, [&](auto W) {
        constexpr int CW = decltype(W)::value;
        if constexpr (CW % 256 == 0)
            hipLaunchKernelGGL((vbm::layernorm_kernel<CW>), dim3((M + 3) / 4), dim3(256), 0, st, resid, g, b, LN_EPS, M, m->L, m->LZ, m->F, xn, map, feat,
                               xb, rstd, mean);
        else      // 384, 192: float2 / float per lane (vb_misc.h)
            hipLaunchKernelGGL((vbm::layernorm_small_kernel<CW>), dim3((M + 3) / 4), dim3(256), 0, st, resid, g, b, LN_EPS, M, m->L, m->LZ, m->F, xn, map,
                               feat, xb, rstd, mean);
    });
    VB_HIP(hipGetLastError());
    return VT_OK;
}

// What an entry addresses for the frame slice [f0, f0 + B) of a batch of Bt frames (vb_api.h Slice; none: the whole batch from frame 0):
// the slice's first token row, its CU budget and every workspace at that frame.
struct SliceView {
    size_t f0, r0;           // first frame, first token row
    int cus;                 // workgroups of a persistent kernel (0 = one per CU)
    long long Bt;            // frames of the whole batch: the stride of tower-major buffers
    bf16 *xn, *qk, *vt, *ao, *hid, *map[5];      // vt: [frame][C][L]; map[0..3]: the head's padded maps, map[4]: conv4's dense output
    float *resid, *rstd, *rmean;
    vbg::f2* stats;
    int ldstats;
    SliceView(const VbModel* m, int B, const vb::Slice* sl)
        : f0(sl ? sl->f0 : 0), r0(f0 * m->L), cus(sl ? sl->cus : 0), Bt(sl ? sl->Btot : B), xn(m->xn.p + r0 * m->C), qk(m->qk.p + r0 * 2 * m->C),
          vt(m->vt.p + r0 * m->C), ao(m->ao.p + r0 * m->C), hid(m->hid.p + r0 * m->HID), resid(m->resid.p + r0 * m->C), rstd(m->rstd.p + r0),
          rmean(m->rmean.p + r0), stats(m->stats.p + r0), ldstats((int)(m->stats.n / m->stat_p())) {
        const size_t P2 = (size_t)(m->F + 2) * (m->F + 2);
        for (int i = 0; i < 4; ++i) map[i] = m->map[i].p + f0 * P2 * m->head_ch(i);
        map[4] = m->t4.p + f0 * (size_t)m->LX * HEAD_CH[4];
    }
    // a GEMM that writes residual rows also leaves their bf16 copy and LayerNorm statistics (the folded LayerNorms, vb_gemm.h)
    void stats_of(vbg::Args& a) const { a.xb = xn; a.stats = stats; a.ldstats = ldstats; }
};

// The patch GEMMs' operand rows [rows][PATCH_K] of a slice.  At widths of at least PATCH_K they lie in a workspace of the width's own rows (ao,
// folded: xn receives the tokens' bf16 copy from the GEMM epilogue; else xn); a narrower model's rows (384, 192) are shorter than an operand
// row, so there the operand lies in the MLP's hidden rows (HID = 4 C >= PATCH_K), idle until the first fc1.
bf16* patch_operand(const VbModel* m, const SliceView& v) {
    static_assert(4 * C_TINY >= PATCH_K, "the hidden rows hold an operand row");
    return m->C >= PATCH_K ? (m->fold ? v.ao : v.xn) : v.hid;
}

int run_finalize(const VbModel* m, const SliceView& v, int M, hipStream_t st, const Err& E) {
    dispatch_width(m->C, [&](auto W) {
        hipLaunchKernelGGL(vbm::ln_finalize_kernel<decltype(W)::value / 64>, dim3((M + 255) / 256), dim3(256), 0, st, v.stats, v.ldstats, M, LN_EPS, v.rstd,
                           v.rmean);
    });
    VB_HIP(hipGetLastError());
    return VT_OK;
}

// LayerNorm(gamma, beta) folded into the Linear(W [N][K], b) that consumes it, in double (vb_gemm.h header):
//     W'[n][k] = W[n][k] gamma[k] - mean_k(W[n][.] gamma[.]),   b'[n] = b[n] + sum_k W[n][k] beta[k]
void fold_layernorm(std::vector<float>& w, std::vector<float>& b, const float* gamma, const float* beta, int N, int K) {
    for (int n = 0; n < N; ++n) {
        float* row = w.data() + (size_t)n * K;
        double sb = 0.0, sg = 0.0;
        for (int k = 0; k < K; ++k) { sb += (double)row[k] * beta[k]; sg += (double)row[k] * gamma[k]; }
        const double mu = sg / K;
        for (int k = 0; k < K; ++k) row[k] = (float)((double)row[k] * gamma[k] - mu);
        b[n] = (float)((double)b[n] + sb);
    }
}

// Preprocessor.process (lib/test/tracker/data_utils.py:11-17: / 255, - mean, / std) folded into the patch embedding of the uint8 search
// patch, in double: against the byte p itself
//     W'[n][c,r,s] = W[n][c,r,s] / (255 std_c),      b'[n] = b[n] - sum W mean_c / std_c
// and wsum[n] = sum W'[n][.] from the UNROUNDED W': what an operand p - ctr adds to the bias, ctr wsum[n].  Both images of the uint8 patch
// weights are built from it (fold_patch_u8: bf16, centred; build_f32_patch_u8: three pieces, uncentred).
struct PatchFold {
    std::vector<float> w;              // W' [C][PATCH_K]
    std::vector<double> bias, wsum;    // [C]
};
PatchFold fold_preprocessor(const VbModel* m) {
    const int C = m->C;
    PatchFold f{std::vector<float>((size_t)C * PATCH_K), std::vector<double>(C), std::vector<double>(C)};
    double k255[3], ms[3];
    for (int c = 0; c < 3; ++c) { k255[c] = 1.0 / (255.0 * (double)m->norm_std[c]); ms[c] = (double)m->norm_mean[c] / (double)m->norm_std[c]; }
    for (int n = 0; n < C; ++n) {
        const float* row = m->h_wpatch.data() + (size_t)n * PATCH_K;
        double sm = 0, sw = 0;
        for (int k = 0; k < PATCH_K; ++k) {
            const int c = k >> 8;
            const double wd = (double)row[k] * k255[c];
            sm += (double)row[k] * ms[c];
            sw += wd;
            f.w[(size_t)n * PATCH_K + k] = (float)wd;
        }
        f.bias[n] = (double)m->h_bpatch[n] - sm;
        f.wsum[n] = sw;
    }
    return f;
}

// The patch GEMM's centring constants, [L]: a token row is patches W^T + bias + pos row; what is known of its mean before the GEMM runs is
// mean(bias) + mean(pos row) (the projection of a normalised patch is zero-mean over channels to first order).  bias_sum: over channels
int upload_centring(Buf<float>& d, const std::vector<float>& pos, int C, double bias_sum, const Err& E) {
    std::vector<float> cpos(pos.size() / C);
    for (size_t t = 0; t < cpos.size(); ++t) {
        double s = 0;
        for (int k = 0; k < C; ++k) s += pos[t * C + k];
        cpos[t] = (float)((s + bias_sum) / C);
    }
    return upload_f32(d, cpos.data(), cpos.size(), E);
}

// ---- the fp32-equivalent mode: weight images and workspaces
// an f32 tensor [rows][K] as its expanded image [rows + pad_rows zero rows][terms K] (vbf::expand_weight_kernel), through a staging upload
int expand_upload(Buf<bf16>& d, const float* h, size_t rows, int K, int terms, size_t pad_rows, const Err& E) {
    Buf<float> stage;
    int rc;
    if ((rc = ensure(d, (rows + pad_rows) * terms * K, E)) || (rc = upload(stage, h, rows * K, E))) return rc;
    if (pad_rows) VB_HIP(hipMemset(d.p + rows * terms * K, 0, pad_rows * terms * K * sizeof(bf16)));
    hipLaunchKernelGGL(vbf::expand_weight_kernel, dim3(grid256(rows * K / 4)), dim3(256), 0, 0, stage.p, d.p, rows, K, terms);
    VB_HIP(hipGetLastError());
    VB_HIP(hipDeviceSynchronize());
    return VT_OK;
}
size_t pad_rows256(int N) { return (size_t)((N + 255) / 256 * 256 - N); }

// The uint8 form of the patch weights for the mode: uncentred (the operand is the byte itself, exact in one piece) and kept to fp32 by the
// three weight pieces
int build_f32_patch_u8(VbModel* m, const Err& E) {
    const PatchFold f = fold_preprocessor(m);
    const std::vector<float> b(f.bias.begin(), f.bias.end());
    if (int rc = expand_upload(m->f32.wpatch_u8, f.w.data(), m->C, PATCH_K, 3, pad_rows256(m->C), E)) return rc;
    return upload_f32(m->f32.bpatch_u8, b.data(), b.size(), E);
}

int build_f32_weights(VbModel* m, const Err& E) {
    ModeF32& f = m->f32;
    const int C = m->C, HID = m->HID;
    int rc;
    f.weights = false;
    if ((rc = expand_upload(f.wpatch, m->h_wpatch.data(), C, PATCH_K, 6, pad_rows256(C), E)) || (rc = build_f32_patch_u8(m, E))) return rc;
    for (BlockF& b : f.blk) {
        if ((rc = expand_upload(b.wqkv, b.h_wqkv.data(), 3 * C, C, 6, pad_rows256(3 * C), E)) || (rc = upload_f32(b.bqkv, b.h_bqkv.data(), b.h_bqkv.size(), E)) ||
            (rc = expand_upload(b.wproj, b.h_wproj.data(), C, C, 6, pad_rows256(C), E)) ||
            (rc = expand_upload(b.w1, b.h_w1.data(), HID, C, 6, pad_rows256(HID), E)) || (rc = upload_f32(b.b1, b.h_b1.data(), b.h_b1.size(), E)) ||
            (rc = expand_upload(b.w2, b.h_w2.data(), C, HID, 6, pad_rows256(C), E)))
            return rc;
    }
    for (int li = 0; li < 4; ++li) {      // [rows][tap][cin] -> [rows][tap][6 cin]: a tap's channels are one expanded row
        const int cin = m->head_ch(li);
        if ((rc = expand_upload(f.wc[li], f.h_wc[li].data(), f.h_wc[li].size() / cin, cin, 6, 0, E))) return rc;
    }
    f.weights = true;
    return VT_OK;
}

// the mode's workspaces, all or none; the new GEMM instantiations' dynamic LDS
int alloc_f32_ws(VbModel* m, const Err& E) {
    ModeF32& f = m->f32;
    if (f.ws) return VT_OK;
    const size_t B = (size_t)m->maxB, M = B * m->L, C = (size_t)m->C, HID = (size_t)m->HID, LX = (size_t)m->LX, P2 = (size_t)(m->F + 2) * (m->F + 2);
    using namespace vbg;
    size_t bytes = 0;
    const hipError_t e = alloc_workspaces(      // the maps: zero borders; the kernels write interiors only
        {{f.x6, M * 6 * C}, {f.hid6, M * 6 * HID}, {f.zop6, B * m->LZ * 6 * PATCH_K}, {f.map6[0], B * P2 * 6 * C, true},
         {f.map6[1], 3 * B * P2 * 6 * HEAD_CH[1], true}, {f.map6[2], 3 * B * P2 * 6 * HEAD_CH[2], true}, {f.map6[3], 3 * B * P2 * 6 * HEAD_CH[3], true},
         {f.hid32, M * HID}, {f.feat32, B * LX * C}, {f.tmp32, B * LX * 3 * HEAD_CH[1]}},
        {{kernel_ptr(gemm_kernel<256, 256, 2, 4, A_PLAIN, EPI_F32>), lds_bytes<256, 256>()},
         {kernel_ptr(gemm_kernel<128, 64, 8, 1, A_PLAIN, EPI_F32>), lds_bytes<128, 64>()},
         {kernel_ptr(gemm_kernel<256, 64, 8, 1, A_CONV, EPI_F32>), lds_bytes<256, 64>()},
         {kernel_ptr(gemm_kernel<128, 64, 8, 1, A_CONV, EPI_F32>), lds_bytes<128, 64>()}},
        &bytes);
    if (e != hipSuccess) return E.fail(VT_ERR_HIP, "fp32 mode: workspaces of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e));
    f.ws = true;
    return VT_OK;
}

// The bf16 image.  Its operand is the CENTRED byte p - ctr (vbm::patchify_u8_kernel, ctr = 128): b'[n] + ctr wsum[n] is the bias.  What the
// bf16 rounding of W' then multiplies is p - 128 instead of p: uncentred, the rounding errors of a row of W' meet a common mode of ~2 sigma
// of the patch and the tokens leave the 3.2e-3 the stage is held to (3.3e-3 on noise patches; centred 1.7e-3; the fp32 route 2.3-2.6e-3:
// NOTES R7-1, tests/test_vitb_track_host.py).  Compensating with the ROUNDED weights instead is algebraically the uncentred form again.
// The centring table of the search rows (Args::cm) follows the bias.
int fold_patch_u8(VbModel* m, const Err& E) {
    const int C = m->C;
    const PatchFold f = fold_preprocessor(m);
    std::vector<float> b(C);
    double bsum = 0;
    for (int n = 0; n < C; ++n) {
        const double bd = f.bias[n] + (double)m->u8_centre * f.wsum[n];
        b[n] = (float)bd;
        bsum += bd;
    }
    int rc;
    if ((rc = upload_bf16(m->wpatch_u8, f.w, E, tile_pad(C, PATCH_K))) || (rc = upload_f32(m->bpatch_u8, b.data(), b.size(), E))) return rc;
    if ((rc = upload_centring(m->cpos_u8, m->h_pos, C, bsum, E))) return rc;
    return m->f32.weights ? build_f32_patch_u8(m, E) : VT_OK;      // (vt_set_normalization in fp32 mode: the mode's image follows)
}

}  // namespace

namespace vb {

int set_normalization(VbModel* m, const float* mean3, const float* std3, std::string* err) {
    const Err E{err};
    std::memcpy(m->norm_mean, mean3, 12);
    std::memcpy(m->norm_std, std3, 12);
    return m->loaded ? fold_patch_u8(m, E) : VT_OK;      // before vt_load_weights: remembered, load_weights folds with it
}

static int build_model(const vt_config* cfg, VbModel** out, const Err& E);

// the "got ..." tail of create's / create_vit's refusals (the ViT-Base message names no depth)
static std::string got_config(const vt_config* cfg, bool depth) {
    return "got channels=" + std::to_string(cfg->channels) + " heads=" + std::to_string(cfg->heads) +
           (depth ? " depth=" + std::to_string(cfg->depth) : std::string()) + " head_channels=" + std::to_string(cfg->head_channels) +
           " stride=" + std::to_string(cfg->stride) + " template=" + std::to_string(cfg->template_size) + " search=" + std::to_string(cfg->search_size);
}

// whether a configuration is model point p at one of the two geometries (depth: within the point's range too)
static bool admits(const ModelPoint& p, const vt_config* cfg, bool depth) {
    const bool g256 = cfg->template_size == 128 && cfg->search_size == 256, g384 = cfg->template_size == 192 && cfg->search_size == 384;
    return cfg->channels == p.C && cfg->heads == p.heads && cfg->head_channels == HW && cfg->stride == 16 && (g256 || g384) &&
           (!depth || (cfg->depth >= 1 && cfg->depth <= p.max_depth));
}

int create(const vt_config* cfg, VbModel** out, std::string* err) {
    const Err E{err};
    const bool large = cfg->channels == C_LARGE;
    const ModelPoint& p = POINTS[large ? 1 : 0];
    const std::string unsupported = std::string("unsupported ") + p.name + " configuration: this build implements ";
    if (large && !admits(p, cfg, true))       // vt_create sends only the exact ViT-Large tuple here; the depth is what is left to refuse
        return E.fail(VT_ERR_ARG, unsupported + "CHANNELS=1024, HEADS=16, HEAD.NUM_CHANNELS=256, "
                                  "STRIDE=16, 1 <= depth <= 24, template 128 / search 256 or template 192 / search 384; " + got_config(cfg, true));
    if (!large && !admits(p, cfg, false))
        return E.fail(VT_ERR_ARG, unsupported + "CHANNELS=768, HEADS=12, "
                                  "HEAD.NUM_CHANNELS=256, STRIDE=16, template 128 / search 256 (OSTrack-256) or template 192 / search 384 "
                                  "(OSTrack-384); " + got_config(cfg, false));
    return build_model(cfg, out, E);
}

int create_vit(const vt_config* cfg, VbModel** out, std::string* err) {
    const Err E{err};
    const ModelPoint* p = model_point(cfg->channels);
    if (p && p->vt_create && cfg->heads == p->heads) return create(cfg, out, err);      // the two tuples vt_create knows: its checks, its messages
    if (!p || p->vt_create || !admits(*p, cfg, true))
        return E.fail(VT_ERR_ARG, "unsupported ViT configuration: this build implements (CHANNELS, HEADS) = (192, 3), (384, 6) with 1 <= depth <= 12, "
                                  "(768, 12), (1024, 16) with 1 <= depth <= 24, HEAD.NUM_CHANNELS=256, STRIDE=16, template 128 / search 256 or "
                                  "template 192 / search 384; " + got_config(cfg, true));
    return build_model(cfg, out, E);
}

// the model of a checked configuration: workspace, switches, kernel attributes
static int build_model(const vt_config* cfg, VbModel** out, const Err& E) {
    const bool g384 = cfg->template_size == 192 && cfg->search_size == 384;
    if (cfg->depth < 1 || cfg->depth > 24 || cfg->max_batch < 1) return E.fail(VT_ERR_ARG, "bad depth / max_batch");
    // the EPI_PATCH_ROWS_N epilogue finds a row's frame by a multiply-high that is exact while rows * rows-per-frame < 2^32
    if (g384 && (uint64_t)cfg->max_batch * 576 * 576 >= (1ull << 32)) return E.fail(VT_ERR_ARG, "max_batch too large for the 192 / 384 geometry");
    // the GEMMs address their operands by 32-bit byte offsets from the operand's base: the widest one, the MLP's hidden rows, has to fit
    {
        const uint64_t Lc = (uint64_t)(cfg->template_size / 16) * (cfg->template_size / 16) + (uint64_t)(cfg->search_size / 16) * (cfg->search_size / 16);
        if ((uint64_t)cfg->max_batch * Lc * (4 * (uint64_t)cfg->channels) * 2 >= (1ull << 32))
            return E.fail(VT_ERR_ARG, "max_batch too large: the MLP's hidden rows of a batch must stay below 4 GiB");
    }
    VbModel* m = new VbModel();
    m->cfg = *cfg;
    m->depth = cfg->depth;
    m->maxB = cfg->max_batch;
    m->C = cfg->channels; m->HEADS = cfg->heads; m->HID = 4 * cfg->channels;
    const int C = m->C, HID = m->HID;
    m->blk.resize(m->depth);
    m->g384 = g384;
    m->TZ = cfg->template_size; m->TX = cfg->search_size;
    m->F = m->TX / 16;
    m->LZ = (m->TZ / 16) * (m->TZ / 16); m->LX = m->F * m->F; m->L = m->LZ + m->LX;
    const int L = m->L, LZ = m->LZ, LX = m->LX, F = m->F;
    auto log2_exact = [](int v) { int s = 0; while ((1 << s) < v) ++s; return (1 << s) == v ? s : -1; };
    m->zshift = log2_exact(LZ); m->xshift = log2_exact(LX);
    m->fold = env_int("VB_LN_FOLD", 1) != 0;
    m->center = env_int("VB_LN_CENTER", 1) != 0;
    m->gemm_narrow = env_int("VB_GEMM_NARROW", -1);
    m->narrow_fill = env_int("VB_GEMM_NARROW_FILL", NARROW_FILL);
    m->fused_qkv = env_int("VB_FUSED_QKV", 1) != 0;
    m->u8_centre = env_int("VB_U8_CENTER", 1) != 0 ? 128.f : 0.f;
    m->attn_stream = env_int("VB_ATTN_STREAM", 0) != 0;
    m->ce_plain = env_int("VB_CE_SCORE_PLAIN", 0) != 0;
    const size_t B = (size_t)cfg->max_batch, M = B * L, P2 = (size_t)(F + 2) * (F + 2);
    // the streaming attention kernel's last key chunk reads up to PAD_TOKENS rows (qk) / elements (vt) past a frame's last token: the
    // workspaces carry that tail so the reads stay inside them, and are zero-filled ONCE, here.  Nothing read there is used: the kernel
    // masks those keys' scores and zeroes their V^T columns in registers (vb_attn_stream.h)
    constexpr size_t PAD = vbs::PAD_TOKENS;
    using namespace vbg;
    const hipError_t e = alloc_workspaces(      // zero-filled: the borders of the padded maps (kernels only ever write interiors), and the two tails
        {{m->xn, M * C}, {m->qk, (M + PAD) * 2 * C, true}, {m->vt, M * C + PAD, true}, {m->ao, M * C}, {m->hid, M * HID}, {m->map[0], B * P2 * (size_t)C, true},
         {m->map[1], 3 * B * P2 * HEAD_CH[1], true}, {m->map[2], 3 * B * P2 * HEAD_CH[2], true}, {m->map[3], 3 * B * P2 * HEAD_CH[3], true},
         {m->t4, 3 * B * LX * HEAD_CH[4]}, {m->zop, B * LZ * PATCH_K}, {m->resid, M * C}, {m->rstd, M}, {m->rmean, M}, {m->stats, (size_t)m->stat_p() * M}},
        {{kernel_ptr(gemm_kernel<256, 256, 2, 4, A_PLAIN, EPI_PATCH>), lds_bytes<256, 256>()},
         {kernel_ptr(gemm_kernel<256, 256, 2, 4, A_PLAIN, EPI_PATCH_ROWS>), lds_bytes<256, 256>()},
         {kernel_ptr(gemm_kernel<256, 256, 2, 4, A_PLAIN, EPI_PATCH_ROWS_N>), lds_bytes<256, 256>()},
         {kernel_ptr(gemm_kernel<256, 256, 2, 4, A_PLAIN, EPI_BF16>), lds_bytes<256, 256>()},
         {kernel_ptr(gemm_kernel<256, 256, 2, 4, A_PLAIN, EPI_VT>), lds_bytes<256, 256>()},
         {kernel_ptr(gemm_kernel<256, 256, 2, 4, A_PLAIN, EPI_RESID>), lds_bytes<256, 256>()},
         {kernel_ptr(gemm_kernel<256, 256, 2, 4, A_PLAIN, EPI_GELU>), lds_bytes<256, 256>()},
         {kernel_ptr(gemm_kernel<256, 256, 2, 4, A_CONV, EPI_CONV>), lds_bytes<256, 256>()},
         {kernel_ptr(gemm_kernel<256, 64, 8, 1, A_CONV, EPI_CONV>), lds_bytes<256, 64>()},
         {kernel_ptr(gemm_kernel<128, 64, 8, 1, A_PLAIN, EPI_PATCH>), lds_bytes<128, 64>()},
         {kernel_ptr(gemm_kernel<128, 64, 8, 1, A_PLAIN, EPI_PATCH_ROWS>), lds_bytes<128, 64>()},
         {kernel_ptr(gemm_kernel<128, 64, 8, 1, A_PLAIN, EPI_PATCH_ROWS_N>), lds_bytes<128, 64>()},
         {kernel_ptr(gemm_kernel<128, 64, 8, 1, A_PLAIN, EPI_BF16>), lds_bytes<128, 64>()},
         {kernel_ptr(gemm_kernel<128, 64, 8, 1, A_PLAIN, EPI_RESID>), lds_bytes<128, 64>()},
         {kernel_ptr(gemm_kernel<128, 64, 8, 1, A_PLAIN, EPI_GELU>), lds_bytes<128, 64>()},
         {kernel_ptr(gemm_kernel<128, 64, 8, 1, A_CONV, EPI_CONV>), lds_bytes<128, 64>()},
         {kernel_ptr(vba::attn_kernel<L256, HD>), vba::Geo<L256, HD>::LDS_BYTES},
         {kernel_ptr(vbs::attn_stream_kernel<L256>), vbs::LDS_BYTES},
         {kernel_ptr(vbs::attn_stream_kernel<L384>), vbs::LDS_BYTES},
         {kernel_ptr(vbs::attn_stream_masked_kernel<L256>), vbs::LDS_BYTES},
         {kernel_ptr(vbs::attn_stream_masked_kernel<L384>), vbs::LDS_BYTES},
         {kernel_ptr(vbs::attn_stream_rt_kernel), vbs::LDS_BYTES},
         {kernel_ptr(vbc::ce_score_all_rt_kernel), 16 * L384 * 4},
         {kernel_ptr(vbq::qkv_attn_kernel), vbq::LDS_BYTES},
         {kernel_ptr(vbq::qkv_attn_wide_kernel<C_LARGE>), vbq::LDS_BYTES},
         {kernel_ptr(vbq::qkv_attn_wide_kernel<C_SMALL>), vbq::LDS_BYTES},
         {kernel_ptr(vbq::qkv_attn_wide_kernel<C_TINY>), vbq::LDS_BYTES},
         {kernel_ptr(gemm_kernel<256, 256, 2, 4, A_PLAIN | A_ANYK, EPI_BF16>), lds_bytes<256, 256>()},
         {kernel_ptr(gemm_kernel<256, 256, 2, 4, A_PLAIN | A_ANYK, EPI_VT>), lds_bytes<256, 256>()},
         {kernel_ptr(gemm_kernel<256, 256, 2, 4, A_PLAIN | A_ANYK, EPI_RESID>), lds_bytes<256, 256>()},
         {kernel_ptr(gemm_kernel<256, 256, 2, 4, A_PLAIN | A_ANYK, EPI_GELU>), lds_bytes<256, 256>()}});
    if (e != hipSuccess) {
        destroy(m);
        return E.fail(VT_ERR_HIP, std::string("ViT workspace: ") + hipGetErrorString(e));
    }
    *out = m;
    return VT_OK;
}

void destroy(VbModel* m) { delete m; }      // every Buf frees its own

int check_ce_args(int n, const int32_t* loc, const double* keep_ratio, std::string* err) {
    const Err E{err};
    if (!loc || !keep_ratio) return E.fail(VT_ERR_ARG, "candidate elimination: null loc / keep_ratio");
    if (n < 1) return E.fail(VT_ERR_ARG, "candidate elimination: at least one stage (n >= 1), got n=" + std::to_string(n));
    for (int k = 0; k < n; ++k) {
        if (loc[k] < 0 || (k > 0 && loc[k] <= loc[k - 1]))
            return E.fail(VT_ERR_ARG, "candidate elimination: loc must be strictly increasing block indices >= 0 (stage " + std::to_string(k) + ": " +
                                          std::to_string(loc[k]) + ")");
        if (!(keep_ratio[k] > 0.0 && keep_ratio[k] <= 1.0))
            return E.fail(VT_ERR_ARG, "candidate elimination: keep_ratio must lie in (0, 1] (stage " + std::to_string(k) + ": " + std::to_string(keep_ratio[k]) + ")");
    }
    return VT_OK;
}

int set_candidate_elimination(VbModel* m, int n, const int32_t* loc, const double* keep_ratio, const uint8_t* template_rows, std::string* err) {
    const Err E{err};
    if (int rc = check_ce_args(n, loc, keep_ratio, err)) return rc;
    if (m->C != C_BASE) return E.fail(VT_ERR_ARG, "candidate elimination is implemented for ViT-Base models (channels 768) only");
    if (m->precision == VT_PRECISION_FP32)
        return E.fail(VT_ERR_STATE, "candidate elimination and fp32 mode exclude each other: this model is in fp32 mode (vt_set_precision)");
    if (n > m->depth || loc[n - 1] >= m->depth)
        return E.fail(VT_ERR_ARG, "candidate elimination: " + std::to_string(n) + " stages up to block " + std::to_string(loc[n - 1]) + " do not fit depth " +
                                      std::to_string(m->depth) + " (1 <= n <= depth, loc in [0, depth))");
    std::vector<int32_t> rows;
    for (int r = 0; r < m->LZ; ++r)
        if (!template_rows || template_rows[r]) rows.push_back(r);
    if (rows.empty()) return E.fail(VT_ERR_ARG, "candidate elimination: template_rows selects no template row");
    std::vector<int> keep(n);
    int prev = m->LX, first = -1;
    for (int k = 0; k < n; ++k) {       // math.ceil(keep_ratio * lens_s) of attn_blocks.py:39, the product in double
        keep[k] = std::min(prev, std::max(1, (int)std::ceil(keep_ratio[k] * (double)prev)));
        if (keep[k] < prev && first < 0) first = loc[k];
        prev = keep[k];
    }
    VB_HIP(hipDeviceSynchronize());      // no step may be reading the buffers that are about to be replaced
    // an earlier configuration is gone from here on: if an allocation below fails the model is a plain one, never old stages on new buffers
    m->ce_set = false;
    m->ce_first = -1;
    m->ce_loc.clear();
    m->ce_keep.clear();
    const size_t B = (size_t)m->maxB, W = (size_t)m->ce_words(), LX = (size_t)m->LX;
    auto fresh = [](auto& buf, size_t count, int byte) {
        buf.release();
        hipError_t e = buf.alloc(count);
        return e != hipSuccess ? e : hipMemset(buf.p, byte, count * sizeof(*buf.p));
    };
    VB_HIP(fresh(m->ce_bits, (size_t)n * B * W, 0));
    VB_HIP(fresh(m->ce_removed, B * LX, 0));
    VB_HIP(fresh(m->ce_scores, (size_t)n * B * LX, 0xff));      // NaN: what a stage that never runs (a no-op) reports
    VB_HIP(fresh(m->ce_part, B * (size_t)m->HEADS * LX, 0));
    m->ce_index_off.assign(n, 0);
    size_t nindex = 0;
    for (int k = 0; k < n; ++k) { m->ce_index_off[k] = nindex; nindex += B * (size_t)keep[k]; }
    VB_HIP(fresh(m->ce_index, nindex, 0));
    VB_HIP(fresh(m->ce_src, B * LX, 0));
    VB_HIP(fresh(m->ce_inv, B * LX, 0));
    if (int rc = upload(m->ce_rows, rows.data(), rows.size(), E)) return rc;
    m->ce_loc.assign(loc, loc + n);
    m->ce_keep = keep;
    m->ce_nrows = (int)rows.size();
    m->ce_first = first;
    m->ce_set = true;
    return VT_OK;
}

int set_ce_form(VbModel* m, int form, std::string* err) {
    const Err E{err};
    if (m->C != C_BASE) return E.fail(VT_ERR_ARG, "candidate elimination is implemented for ViT-Base models (channels 768) only");
    if (form != VT_CE_MASKED && form != VT_CE_COMPACT)
        return E.fail(VT_ERR_ARG, "candidate elimination form " + std::to_string(form) + ": VT_CE_MASKED (0) or VT_CE_COMPACT (1)");
    m->ce_form = form;
    return VT_OK;
}

int ce_result(VbModel* m, int B, hipStream_t st, uint8_t* removed_stage, float* scores, std::string* err) {
    const Err E{err};
    if (!m->ce_set) return E.fail(VT_ERR_STATE, "vt_set_candidate_elimination has not been called");
    if (B < 1 || B > m->maxB) return E.fail(VT_ERR_STATE, "batch " + std::to_string(B) + " outside [1, max_batch=" + std::to_string(m->maxB) + "]");
    const size_t LX = (size_t)m->LX;
    if (removed_stage) VB_HIP(hipMemcpyAsync(removed_stage, m->ce_removed.p, (size_t)B * LX, hipMemcpyDeviceToDevice, st));
    if (scores)
        VB_HIP(hipMemcpy2DAsync(scores, (size_t)B * LX * 4, m->ce_scores.p, (size_t)m->maxB * LX * 4, (size_t)B * LX * 4, m->ce_loc.size(),
                                hipMemcpyDeviceToDevice, st));
    return VT_OK;
}

// Key layout: the reference's OSTrack ckpt['net'] -- backbone.{patch_embed.proj, pos_embed_z, pos_embed_x, blocks.N.*, norm},
// box_head.* (lib/models/ostrack/vit.py:94-139, base_backbone.py:83-84, lib/models/layers/head.py:98-128).
int load_weights(VbModel* m, const TensorMap& tm, std::string* err) {
    const Err E{err};
    int rc;
    const float* p;
    const std::string bb = "backbone.";
    const int L = m->L, LZ = m->LZ, LX = m->LX, C = m->C, HID = m->HID;
    const float *wp, *bp;
    if ((rc = load_bf16(m->wpatch, tm, bb + "patch_embed.proj.weight", (int64_t)C * PATCH_K, E, &wp, tile_pad(C, PATCH_K)))) return rc;
    if ((rc = load_f32(m->bpatch, tm, bb + "patch_embed.proj.bias", C, E, &bp))) return rc;
    m->h_wpatch.assign(wp, wp + (size_t)C * PATCH_K);
    m->h_bpatch.assign(bp, bp + C);
    m->h_pos.resize((size_t)L * C);
    if ((rc = need(tm, bb + "pos_embed_z", (int64_t)LZ * C, &p, E))) return rc;
    std::memcpy(m->h_pos.data(), p, (size_t)LZ * C * 4);
    if ((rc = need(tm, bb + "pos_embed_x", (int64_t)LX * C, &p, E))) return rc;
    std::memcpy(m->h_pos.data() + (size_t)LZ * C, p, (size_t)LX * C * 4);
    if ((rc = upload_f32(m->pos, m->h_pos.data(), m->h_pos.size(), E))) return rc;
    double bsum = 0;
    for (int k = 0; k < C; ++k) bsum += bp[k];
    if ((rc = upload_centring(m->cpos, m->h_pos, C, bsum, E)) || (rc = fold_patch_u8(m, E))) return rc;
    const float scale = 1.0f / std::sqrt((float)HD);     // 0.125: a power of two, folding it into W_q / b_q is exact
    m->f32.blk.resize(m->depth);
    m->f32.weights = false;
    for (int i = 0; i < m->depth; ++i) {
        BlockW& b = m->blk[i];
        BlockF& bf = m->f32.blk[i];
        const std::string pre = bb + "blocks." + std::to_string(i) + ".";
        const float *g1, *be1, *g2, *be2;
        if ((rc = load_f32(b.ln1g, tm, pre + "norm1.weight", C, E, &g1)) || (rc = load_f32(b.ln1b, tm, pre + "norm1.bias", C, E, &be1))) return rc;
        if ((rc = load_f32(b.ln2g, tm, pre + "norm2.weight", C, E, &g2)) || (rc = load_f32(b.ln2b, tm, pre + "norm2.bias", C, E, &be2))) return rc;
        if ((rc = load_f32(b.bproj, tm, pre + "attn.proj.bias", C, E)) || (rc = load_f32(b.b2, tm, pre + "mlp.fc2.bias", C, E))) return rc;
        // a Linear behind a LayerNorm: the norm folded in (VB_LN_FOLD), its first `nscaled` output rows times the attention scale
        auto folded = [&](const std::string& name, int N, const float* g, const float* be, int nscaled, Buf<bf16>& W, Buf<float>& Bv, size_t pad,
                          std::vector<float>& hw, std::vector<float>& hb) {
            const float *pw, *pb;
            if ((rc = need(tm, pre + name + ".weight", (int64_t)N * C, &pw, E)) || (rc = need(tm, pre + name + ".bias", N, &pb, E))) return rc;
            std::vector<float> w(pw, pw + (size_t)N * C), bias(pb, pb + N);
            hw = w; hb = bias;      // the fp32-equivalent mode's: unfolded, scaled
            for (size_t k = 0; k < (size_t)nscaled * C; ++k) hw[k] *= scale;
            for (int k = 0; k < nscaled; ++k) hb[k] *= scale;
            if (m->fold) fold_layernorm(w, bias, g, be, N, C);
            for (size_t k = 0; k < (size_t)nscaled * C; ++k) w[k] *= scale;
            for (int k = 0; k < nscaled; ++k) bias[k] *= scale;
            if ((rc = upload_bf16(W, w, E, pad))) return rc;
            return upload_f32(Bv, bias.data(), bias.size(), E);
        };
        const float *hproj, *hfc2;
        if ((rc = folded("attn.qkv", 3 * C, g1, be1, C, b.wqkv, b.bqkv, tile_pad(C, C), bf.h_wqkv, bf.h_bqkv))) return rc;      // the v GEMM's N = C rows end the matrix
        if ((rc = load_bf16(b.wproj, tm, pre + "attn.proj.weight", (int64_t)C * C, E, &hproj, tile_pad(C, C)))) return rc;
        if ((rc = folded("mlp.fc1", HID, g2, be2, 0, b.w1, b.b1, tile_pad(HID, C), bf.h_w1, bf.h_b1))) return rc;
        if ((rc = load_bf16(b.w2, tm, pre + "mlp.fc2.weight", (int64_t)HID * C, E, &hfc2, tile_pad(C, HID)))) return rc;
        bf.h_wproj.assign(hproj, hproj + (size_t)C * C);
        bf.h_w2.assign(hfc2, hfc2 + (size_t)HID * C);
    }
    if ((rc = load_f32(m->ng, tm, bb + "norm.weight", C, E)) || (rc = load_f32(m->nb, tm, bb + "norm.bias", C, E))) return rc;
    // ---- head: Conv3x3(+bias) + BatchNorm(eval, eps 1e-5) folded in double (head.py:8-21), weights as [cout][tap][cin]
    const char* towers[3] = {"ctr", "offset", "size"};
    for (int li = 0; li < 4; ++li) {
        const int cin = m->head_ch(li), cout = HEAD_CH[li + 1], K = 9 * cin;
        const int rows = head_rows(li, cout);
        std::vector<float> w((size_t)3 * rows * K, 0.f), bias((size_t)3 * cout);
        for (int t = 0; t < 3; ++t) {
            const std::string cn = std::string("box_head.conv") + std::to_string(li + 1) + "_" + towers[t];
            const char* keys[6] = {".0.weight", ".0.bias", ".1.weight", ".1.bias", ".1.running_mean", ".1.running_var"};
            const float* t6[6];
            for (int k = 0; k < 6; ++k)
                if ((rc = need(tm, cn + keys[k], k ? cout : (int64_t)cout * cin * 9, &t6[k], E))) return rc;
            const float *pw = t6[0], *pb = t6[1], *g = t6[2], *beta = t6[3], *mu = t6[4], *var = t6[5];
            for (int o = 0; o < cout; ++o) {
                const double k = (double)g[o] / std::sqrt((double)var[o] + 1e-5);
                float* dst = w.data() + ((size_t)t * rows + o) * K;
                for (int c = 0; c < cin; ++c)
                    for (int tap = 0; tap < 9; ++tap) dst[(size_t)tap * cin + c] = (float)((double)pw[((size_t)o * cin + c) * 9 + tap] * k);
                bias[(size_t)t * cout + o] = (float)(((double)pb[o] - (double)mu[o]) * k + (double)beta[o]);
            }
        }
        if ((rc = upload_bf16(m->wc[li], w, E))) return rc;
        if ((rc = upload_f32(m->bc[li], bias.data(), bias.size(), E))) return rc;
        m->f32.h_wc[li] = std::move(w);
    }
    {
        const int CW = HEAD_CH[4];
        std::vector<float> w5((size_t)5 * CW), b5(5);
        int row = 0;
        for (int t = 0; t < 3; ++t) {
            const int nout = t == 0 ? 1 : 2;
            const std::string c5 = std::string("box_head.conv5_") + towers[t];
            if ((rc = need(tm, c5 + ".weight", (int64_t)nout * CW, &p, E))) return rc;
            std::memcpy(w5.data() + (size_t)row * CW, p, (size_t)nout * CW * 4);
            if ((rc = need(tm, c5 + ".bias", nout, &p, E))) return rc;
            std::memcpy(b5.data() + row, p, nout * 4);
            row += nout;
        }
        if ((rc = upload_f32(m->w5, w5.data(), w5.size(), E))) return rc;
        if ((rc = upload_f32(m->b5, b5.data(), 5, E))) return rc;
    }
    m->loaded = true;
    if (m->precision == VT_PRECISION_FP32 && (rc = build_f32_weights(m, E))) { m->loaded = false; return rc; }
    return VT_OK;
}

static int check(VbModel* m, int B, const Err& E) {
    if (!m->loaded) return E.fail(VT_ERR_STATE, "vt_load_weights has not been called");
    if (B < 1 || B > m->maxB) return E.fail(VT_ERR_STATE, "batch " + std::to_string(B) + " outside [1, max_batch=" + std::to_string(m->maxB) + "]");
    return VT_OK;
}

static int check_slice(VbModel* m, int B, const Slice* sl, const Err& E) {
    if (sl && (sl->Btot < 1 || sl->Btot > m->maxB || sl->f0 + (size_t)B > (size_t)sl->Btot))
        return E.fail(VT_ERR_STATE, "frame slice outside the batch");
    return VT_OK;
}

// ------------------------------------------------------------------------------ the fp32-equivalent mode
int precision(const VbModel* m) { return m->precision; }

int set_precision(VbModel* m, int prec, std::string* err) {
    const Err E{err};
    if (prec != VT_PRECISION_BF16 && prec != VT_PRECISION_FP32)
        return E.fail(VT_ERR_ARG, "precision " + std::to_string(prec) + ": VT_PRECISION_BF16 (0) or VT_PRECISION_FP32 (1)");
    if (prec == VT_PRECISION_FP32 && m->ce_set)
        return E.fail(VT_ERR_STATE, "fp32 mode and candidate elimination exclude each other: this model has candidate elimination set");
    VB_HIP(hipDeviceSynchronize());      // no step may be running on the buffers of the other mode
    if (prec == VT_PRECISION_FP32) {
        if (int rc = alloc_f32_ws(m, E)) return rc;
        if (m->loaded && !m->f32.weights)
            if (int rc = build_f32_weights(m, E)) return rc;
    }
    m->precision = prec;
    return VT_OK;
}

namespace {
// the bytes of an expanded operand one GEMM launch of the mode may span: below the 4 GiB its 32-bit byte offsets reach
constexpr unsigned long long F32_OPERAND_BYTES = (1ull << 32) - (1ull << 20);
// The GEMMs address an operand by 32-bit offsets from its base (vb_gemm.h), and an expanded operand of a whole batch can pass 4 GiB (fc2's:
// rows x 6 HID x 2 bytes -- 9.1 GB for ViT-Large at 192 / 384 with 256 frames): a GEMM of the mode runs as launches of at most `most` units
// (rows or frames), each with its operand, residual and output based at its first unit.  body(first, count) is one launch.  Every output
// element keeps its whole sum in one workgroup in the same order wherever its tile lies, so the chunking changes no bit (tests: B = 66
// against frames one at a time).
template <typename Body>
int for_chunks(int units, int most, Body&& body) {
    for (int u0 = 0; u0 < units; u0 += most)
        if (int rc = body(u0, std::min(most, units - u0))) return rc;
    return VT_OK;
}
// what an fp32-mode entry addresses for a frame slice (SliceView holds the residual stream and the slice itself)
struct SliceF32 {
    bf16 *x6, *hid6, *zop6, *map6[4];
    float *hid32, *feat32, *tmp32;
    SliceF32(const VbModel* m, const SliceView& v) {
        const ModeF32& f = m->f32;
        const size_t P2 = (size_t)(m->F + 2) * (m->F + 2);
        x6 = f.x6.p + v.r0 * 6 * m->C; hid6 = f.hid6.p + v.r0 * 6 * m->HID; zop6 = f.zop6.p + v.f0 * m->LZ * 6 * PATCH_K;
        for (int i = 0; i < 4; ++i) map6[i] = f.map6[i].p + v.f0 * P2 * 6 * m->head_ch(i);
        hid32 = f.hid32.p + v.r0 * m->HID; feat32 = f.feat32.p + v.f0 * m->LX * m->C; tmp32 = f.tmp32.p + v.f0 * m->LX * 3 * HEAD_CH[1];
    }
    // the patch GEMMs' expanded operand rows [rows][6 x 768]: in the width's own rows, or (384, 192) in the hidden rows
    bf16* patch_operand(const VbModel* m) const { return m->C >= PATCH_K ? x6 : hid6; }
};

// one token kind's rows of an fp32 crop batch (B, 3, T, T) as a dense operand: bf16 [rows][PATCH_K] (patchify_kernel with no template, Tz = 0,
// walks the crops alone) or, in fp32 mode, expanded [rows][6 PATCH_K]
int patchify_crop(const VbModel* m, const float* img, int T, int B, bf16* P, hipStream_t st, const Err& E) {
    const dim3 grid(grid256((size_t)B * (T / 16) * (T / 16) * 96));
    if (m->precision == VT_PRECISION_FP32) hipLaunchKernelGGL(vbf::patchify_split_kernel, grid, dim3(256), 0, st, img, P, B, T);
    else hipLaunchKernelGGL(vbm::patchify_kernel, grid, dim3(256), 0, st, nullptr, img, P, B, 0, T);
    VB_HIP(hipGetLastError());
    return VT_OK;
}
// the search rows from the uint8 patch: bf16 [rows][PATCH_K] of centred bytes, or [rows][3 PATCH_K] of the bytes themselves
int patchify_u8(const VbModel* m, const unsigned char* xu8, int B, bf16* P, hipStream_t st, const Err& E) {
    const dim3 grid(grid256((size_t)B * m->LX * 16));
    if (m->precision == VT_PRECISION_FP32) hipLaunchKernelGGL(vbf::patchify_u8_split_kernel, grid, dim3(256), 0, st, xu8, P, B, m->TX);
    else hipLaunchKernelGGL(vbm::patchify_u8_kernel, grid, dim3(256), 0, st, xu8, P, B, m->TX, m->u8_centre);
    VB_HIP(hipGetLastError());
    return VT_OK;
}

int run_layernorm_split(const VbModel* m, const float* resid, const float* g, const float* b, int M, hipStream_t st, bf16* xs, float* feat, const Err& E) {
    dispatch_width(m->C, [&](auto W) {
        hipLaunchKernelGGL((vbm::layernorm_split_kernel<decltype(W)::value>), dim3((M + 3) / 4), dim3(256), 0, st, resid, g, b, LN_EPS, M, m->L, m->LZ, xs, feat);
    });
    VB_HIP(hipGetLastError());
    return VT_OK;
}

// f32 rows -> a zero-bordered map of expanded pixels, `towers` of them (vbf::map_split_kernel)
int run_map_split(const float* src, size_t src_tower, int ld, bf16* dst, size_t dst_tower, int towers, int B, int F, int C, bool relu, hipStream_t st,
                  const Err& E) {
    hipLaunchKernelGGL(vbf::map_split_kernel, dim3(grid256((size_t)B * F * F * (C / 8)), towers), dim3(256), 0, st, src, src_tower, ld, dst, dst_tower, B, F, C,
                       relu ? 1 : 0);
    VB_HIP(hipGetLastError());
    return VT_OK;
}

// The stem on dense operands of one token kind each: the z GEMM, then the x GEMM, onto the token rows of the residual stream.  What the
// two precisions differ in:
struct StemRoute {
    bf16 *zop_given, *xop;         // where a given template's / the search crops' operand rows are written
    const bf16* zop_cached;        // vt_set_template's rows
    int Kz, Kx;                    // operand depth: PATCH_K in bf16; six terms from an fp32 crop, three from a uint8 patch in fp32 mode
    const bf16 *Wz, *Wx;
    const float *bz, *bx;
    const float *cmz, *cmx;        // the rows' centring constants (folded LayerNorm, VB_LN_CENTER), or nullptr
    bool stats;                    // the GEMMs leave the rows' bf16 copy and statistics, ln_finalize follows (folded LayerNorm)
    bool chunked;                  // launches of whole frames below F32_OPERAND_BYTES (no bf16 copy and no statistics behind them)
};
StemRoute stem_route(const VbModel* m, const SliceView& v, int B, bool u8) {
    const size_t zrows = (size_t)B * m->LZ;
    StemRoute r{};
    r.bz = m->bpatch.p;
    if (m->precision == VT_PRECISION_FP32) {
        const SliceF32 w(m, v);
        const ModeF32& f = m->f32;
        r.zop_given = w.patch_operand(m);
        r.xop = r.zop_given + zrows * 6 * PATCH_K;
        r.zop_cached = w.zop6;
        r.Kz = 6 * PATCH_K; r.Kx = u8 ? 3 * PATCH_K : 6 * PATCH_K;
        r.Wz = f.wpatch.p; r.Wx = u8 ? f.wpatch_u8.p : f.wpatch.p;
        r.bx = u8 ? f.bpatch_u8.p : m->bpatch.p;
        r.chunked = true;
        return r;
    }
    // B * LX dense rows inside the slice's B * L (as vb::stem's operand); in the hidden rows (narrow models) behind the B * LZ rows of a given
    // template.  A given template goes to the hidden rows, not through the cache: such a call leaves vt_set_template's rows alone
    r.zop_given = v.hid;
    r.xop = patch_operand(m, v) + (m->C >= PATCH_K ? (size_t)0 : zrows * PATCH_K);
    r.zop_cached = m->zop.p + v.f0 * m->LZ * PATCH_K;
    r.Kz = r.Kx = PATCH_K;
    r.Wz = m->wpatch.p; r.Wx = u8 ? m->wpatch_u8.p : m->wpatch.p;
    r.bx = u8 ? m->bpatch_u8.p : m->bpatch.p;
    if (m->fold && m->center) { r.cmz = m->cpos.p; r.cmx = u8 ? m->cpos_u8.p : m->cpos.p; }
    r.stats = m->fold;
    return r;
}

int run_stem_rows(VbModel* m, ZSrc zsrc, const float* z, const float* x, const unsigned char* xu8, int B, hipStream_t st, const SliceView& v, const Err& E) {
    int rc;
    const int L = m->L, LZ = m->LZ, LX = m->LX, C = m->C;
    const StemRoute r = stem_route(m, v, B, xu8 != nullptr);
    if (zsrc == Z_GIVEN && (rc = patchify_crop(m, z, m->TZ, B, r.zop_given, st, E))) return rc;
    if ((rc = xu8 ? patchify_u8(m, xu8, B, r.xop, st, E) : patchify_crop(m, x, m->TX, B, r.xop, st, E))) return rc;
    vbg::Args a{};
    a.resid = v.resid; a.pos = m->pos.p; a.N = C; a.L = L;
    if (r.stats) v.stats_of(a);
    // operand rows -> (frame, token): a shift at 64 / 256 rows per frame, the rows themselves at 144 / 576 (EPI_PATCH_ROWS_N)
    auto rows_gemm = [&](const vbg::Args& whole, int rows, int shift) {
        const int fmax = r.chunked ? std::max(1, (int)(F32_OPERAND_BYTES / ((unsigned long long)rows * whole.K * 2))) : B;
        return for_chunks(B, fmax, [&](int f0, int nf) {
            vbg::Args g = whole;
            g.X = whole.X + (size_t)f0 * rows * whole.K; g.resid = whole.resid + (size_t)f0 * L * C; g.M = nf * rows;
            g.row_shift = shift < 0 ? rows : shift;
            return shift < 0 ? launch_tile<vbg::A_PLAIN, vbg::EPI_PATCH_ROWS_N>(m, g, 1, st, E, v.cus)
                             : launch_tile<vbg::A_PLAIN, vbg::EPI_PATCH_ROWS>(m, g, 1, st, E, v.cus);
        });
    };
    if (zsrc != Z_NONE) {
        vbg::Args az = a;
        az.X = zsrc == Z_GIVEN ? r.zop_given : r.zop_cached; az.W = r.Wz; az.bias = r.bz; az.cm = r.cmz; az.K = r.Kz; az.row_o0 = 0;
        if ((rc = rows_gemm(az, LZ, m->zshift))) return rc;
    }
    a.X = r.xop; a.W = r.Wx; a.bias = r.bx; a.cm = r.cmx; a.K = r.Kx; a.row_o0 = LZ;
    if ((rc = rows_gemm(a, LX, m->xshift))) return rc;
    return r.stats ? run_finalize(m, v, B * L, st, E) : (int)VT_OK;
}
}  // namespace

// vb::blocks in fp32 mode: LayerNorm -> expanded operand -> qkv GEMM (f32 rows) -> f32 attention -> expanded operand -> proj (f32
// read-modify-write) -> LayerNorm -> fc1 (f32 pre-activation) -> exact GELU -> expanded operand -> fc2; the final norm writes f32 features
static int blocks_f32(VbModel* m, int B, int nblocks, hipStream_t st, float* feat_out, float* resid_out, const SliceView& v,
                      const Err& E) {
    int rc;
    const int C = m->C, HID = m->HID, L = m->L, M = B * L;
    const SliceF32 w(m, v);
    float* const qkv = w.hid32;      // [M][3 C] in the hidden rows, idle until fc1
    const int qtiles = (L + vbf::AQ - 1) / vbf::AQ;
    // launches of at most chunk_rows(K) rows (for_chunks)
    auto chunk_rows = [](int K) { return std::max(256, (int)((F32_OPERAND_BYTES / ((unsigned long long)K * 2)) / 256 * 256)); };
    auto resid_gemm = [&](const bf16* X, const bf16* W, const float* bias, int K) {
        return for_chunks(M, chunk_rows(K), [&](int r0, int rows) {
            vbg::Args p{};
            p.X = X + (size_t)r0 * K; p.W = W; p.bias = bias; p.resid = v.resid + (size_t)r0 * C; p.M = rows; p.N = C; p.K = K;
            return launch_tile<vbg::A_PLAIN, vbg::EPI_RESID>(m, p, 1, st, E, v.cus);
        });
    };
    auto f32_gemm = [&](const bf16* W, const float* bias, float* out, int N) {
        const int K = 6 * C;
        return for_chunks(M, chunk_rows(K), [&](int r0, int rows) {
            vbg::Args a{};
            a.X = w.x6 + (size_t)r0 * K; a.W = W; a.bias = bias; a.out = out + (size_t)r0 * N; a.M = rows; a.N = N; a.K = K; a.ldo = N; a.rb = 4;
            return launch_tile<vbg::A_PLAIN, vbg::EPI_F32>(m, a, 1, st, E, v.cus);
        });
    };
    for (int i = 0; i < nblocks; ++i) {
        const BlockW& b = m->blk[i];
        const BlockF& bf = m->f32.blk[i];
        if ((rc = run_layernorm_split(m, v.resid, b.ln1g.p, b.ln1b.p, M, st, w.x6, nullptr, E))) return rc;
        if ((rc = f32_gemm(bf.wqkv.p, bf.bqkv.p, qkv, 3 * C))) return rc;
        hipLaunchKernelGGL(vbf::attn_f32_kernel, dim3(B * m->HEADS * qtiles), dim3(256), 0, st, qkv, w.x6, C, m->HEADS, L, qtiles);
        VB_HIP(hipGetLastError());
        if ((rc = resid_gemm(w.x6, bf.wproj.p, b.bproj.p, 6 * C))) return rc;
        if ((rc = run_layernorm_split(m, v.resid, b.ln2g.p, b.ln2b.p, M, st, w.x6, nullptr, E))) return rc;
        if ((rc = f32_gemm(bf.w1.p, bf.b1.p, w.hid32, HID))) return rc;
        hipLaunchKernelGGL(vbm::gelu_split_kernel, dim3(grid256((size_t)M * (HID / 8))), dim3(256), 0, st, w.hid32, w.hid6, (size_t)M, HID);
        VB_HIP(hipGetLastError());
        if ((rc = resid_gemm(w.hid6, bf.w2.p, b.b2.p, 6 * HID))) return rc;
    }
    if (resid_out) VB_HIP(hipMemcpyAsync(resid_out, v.resid, (size_t)M * C * 4, hipMemcpyDeviceToDevice, st));
    if ((rc = run_layernorm_split(m, v.resid, m->ng.p, m->nb.p, M, st, nullptr, w.feat32, E))) return rc;
    if (feat_out) VB_HIP(hipMemcpyAsync(feat_out, w.feat32, (size_t)B * m->LX * C * 4, hipMemcpyDeviceToDevice, st));
    return run_map_split(w.feat32, 0, C, w.map6[0], 0, 1, B, m->F, C, false, st, E);
}

// vb::head in fp32 mode: the towers as A_CONV GEMMs on maps of expanded pixels (six k-ranges per tap) with f32 outputs; a conv's ReLU is
// applied where its output is expanded for the next one (conv4's: in the 1 x 1 tail)
static int head_f32(VbModel* m, const float* feat_in, int B, hipStream_t st, float* score, float* size, float* offset, const SliceView& v, const Err& E) {
    int rc;
    const int LX = m->LX, F = m->F, M = B * LX, C = m->C;
    const SliceF32 w(m, v);
    const long long Bt = v.Bt, P2 = (long long)(F + 2) * (F + 2);
    // (a map of expanded pixels is addressed by 32-bit element offsets from the slice's first frame: launches of at most `fmax` frames, each
    // based at its first frame; the tile is chosen for the whole call, as vt_gemm_form reports it)
    auto conv = [&](const vbg::Args& whole, int groups) {
        const bool narrow = narrow_pick(m, whole.M, whole.N, groups, v.cus);
        const int fmax = std::max(1, (int)((1ull << 31) / ((unsigned long long)P2 * whole.C) - 1));
        return for_chunks(B, fmax, [&](int f0, int nf) {
            vbg::Args a = whole;
            a.X = whole.X + (size_t)f0 * P2 * whole.C; a.M = nf * LX;
            a.out = static_cast<float*>(whole.out) + (size_t)f0 * LX * whole.ldo;
            return narrow ? launch_gemm<128, 64, 8, 1, vbg::A_CONV, vbg::EPI_F32>(a, groups, st, E, v.cus)
                          : launch_gemm<256, 64, 8, 1, vbg::A_CONV, vbg::EPI_F32>(a, groups, st, E, v.cus);
        });
    };
    if (feat_in && (rc = run_map_split(feat_in, 0, C, w.map6[0], 0, 1, B, F, C, false, st, E))) return rc;
    {   // conv1 of the three towers as one GEMM: N = 3 x 256 dense f32 columns, K = 9 taps x 6 C
        vbg::Args a{};
        a.X = w.map6[0]; a.W = m->f32.wc[0].p; a.bias = m->bc[0].p; a.out = w.tmp32;
        a.M = M; a.N = 3 * HEAD_CH[1]; a.K = 9 * 6 * C; a.ldo = 3 * HEAD_CH[1]; a.C = 6 * C; a.F = F;
        if ((rc = conv(a, 1))) return rc;
        if ((rc = run_map_split(w.tmp32, HEAD_CH[1], 3 * HEAD_CH[1], w.map6[1], (size_t)(Bt * P2 * 6 * HEAD_CH[1]), 3, B, F, HEAD_CH[1], true, st, E))) return rc;
    }
    for (int li = 1; li < 4; ++li) {   // conv2..4: blockIdx.y = tower, f32 outputs [tower][the slice's pixels][cout]
        const int cin = HEAD_CH[li], cout = HEAD_CH[li + 1], rows = head_rows(li, cout);
        vbg::Args a{};
        a.X = w.map6[li]; a.W = m->f32.wc[li].p; a.bias = m->bc[li].p; a.out = w.tmp32;
        a.M = M; a.N = cout; a.K = 9 * 6 * cin; a.ldo = cout; a.C = 6 * cin; a.F = F;
        a.gX = Bt * P2 * 6 * cin; a.gW = (long long)rows * 9 * 6 * cin; a.gBias = cout; a.gOut = (long long)M * cout;
        if ((rc = conv(a, 3))) return rc;
        if (li < 3 && (rc = run_map_split(w.tmp32, (size_t)M * cout, cout, w.map6[li + 1], (size_t)(Bt * P2 * 6 * cout), 3, B, F, cout, true, st, E))) return rc;
    }
    hipLaunchKernelGGL((vbf::conv5_f32_kernel<32>), dim3((M + 255) / 256), dim3(256), 0, st, w.tmp32, m->w5.p, m->b5.p, M, LX, (size_t)M * HEAD_CH[4], score, size,
                       offset);
    VB_HIP(hipGetLastError());
    return VT_OK;
}

int stem(VbModel* m, const float* z, const float* x, int B, hipStream_t st, float* tokens_out, std::string* err, const Slice* sl) {
    const Err E{err};
    int rc = check(m, B, E);
    if (rc || (rc = check_slice(m, B, sl, E))) return rc;
    if (m->precision == VT_PRECISION_FP32) {
        const SliceView v(m, B, sl);
        if ((rc = run_stem_rows(m, Z_GIVEN, z, x, nullptr, B, st, v, E))) return rc;      // one arithmetic for the cached and the given template
        if (tokens_out) VB_HIP(hipMemcpyAsync(tokens_out, v.resid, (size_t)B * m->L * m->C * 4, hipMemcpyDeviceToDevice, st));
        return VT_OK;
    }
    const int L = m->L, M = B * L, C = m->C;
    const SliceView v(m, B, sl);
    bf16* const patches = patch_operand(m, v);
    hipLaunchKernelGGL(vbm::patchify_kernel, dim3(grid256((size_t)M * 96)), dim3(256), 0, st, z, x, patches, B, m->TZ, m->TX);
    VB_HIP(hipGetLastError());
    vbg::Args a{};
    a.X = patches; a.W = m->wpatch.p; a.bias = m->bpatch.p; a.resid = v.resid; a.pos = m->pos.p;
    a.M = M; a.N = C; a.K = PATCH_K; a.L = L;
    if (m->fold) v.stats_of(a);
    if (m->fold && m->center) { a.cm = m->cpos.p; a.cm_mod = L; }
    if ((rc = launch_tile<vbg::A_PLAIN, vbg::EPI_PATCH>(m, a, 1, st, E, v.cus))) return rc;
    if (m->fold && (rc = run_finalize(m, v, M, st, E))) return rc;
    if (tokens_out) VB_HIP(hipMemcpyAsync(tokens_out, v.resid, (size_t)M * C * 4, hipMemcpyDeviceToDevice, st));
    return VT_OK;
}

int set_template(VbModel* m, const float* z, int n, const int32_t* slots, hipStream_t st, std::string* err) {
    const Err E{err};
    int rc = check(m, n, E);
    if (rc) return rc;
    const int TZ = m->TZ;
    const bool f32 = m->precision == VT_PRECISION_FP32;      // the mode caches the expanded operand rows (vb_f32.h)
    const size_t zrow = (size_t)m->LZ * PATCH_K * (f32 ? 6 : 1);
    bf16* const zop = f32 ? m->f32.zop6.p : m->zop.p;
    if (!slots) return patchify_crop(m, z, TZ, n, zop, st, E);
    for (int i = 0; i < n; ++i) {      // a frame's operand rows depend on that frame alone: straight into place
        if (slots[i] < 0 || slots[i] >= m->maxB) return E.fail(VT_ERR_ARG, "template slot outside the batch");
        if ((rc = patchify_crop(m, z + (size_t)i * 3 * TZ * TZ, TZ, 1, zop + (size_t)slots[i] * zrow, st, E))) return rc;
    }
    return VT_OK;
}

int stem_rows(VbModel* m, ZSrc zsrc, const float* z, const float* x, const unsigned char* xu8, int B, hipStream_t st, float* x_tokens_out,
              std::string* err, const Slice* sl) {
    const Err E{err};
    int rc = check(m, B, E);
    if (rc || (rc = check_slice(m, B, sl, E))) return rc;
    if ((x != nullptr) == (xu8 != nullptr)) return E.fail(VT_ERR_ARG, "stem_rows: one of the fp32 crop and the uint8 patch");
    if (xu8 && (reinterpret_cast<uintptr_t>(xu8) & 15)) return E.fail(VT_ERR_ARG, "the uint8 patch must be 16-byte aligned on the ViT-Base path");
    const int L = m->L, LZ = m->LZ, LX = m->LX, C = m->C;
    const SliceView v(m, B, sl);
    if ((rc = run_stem_rows(m, zsrc, z, x, xu8, B, st, v, E))) return rc;
    if (x_tokens_out)
        VB_HIP(hipMemcpy2DAsync(x_tokens_out + (size_t)LZ * C, (size_t)L * C * 4, v.resid + (size_t)LZ * C, (size_t)L * C * 4, (size_t)LX * C * 4, B,
                                hipMemcpyDeviceToDevice, st));
    return VT_OK;
}

// One block's attention into v.ao, in one of four forms:
//   fused (the default at 320 tokens)       vbq::qkv_attn_kernel: projection + attention of a (frame, head) in one workgroup, q / k / v^T never leave the CU
//   otherwise qk GEMM + v GEMM (V^T) and    vbs::attn_stream_kernel<720> (the 384 geometry), vbs::attn_stream_kernel<320> (VB_ATTN_STREAM) or
//                                           vba::attn_kernel<320, 64>
// ce: a block from the first candidate-elimination stage on -- always qk GEMM + v GEMM + the streaming kernel at either geometry (the stage's
// score reads the q | k rows the qk GEMM leaves in v.qk); keys: the slice's key bitmap (vb_ce.h), nullptr = every key (the first stage's block).
// Lp > 0: behind a compacting stage (the compact form) -- the GEMMs on the slice's B * Lp dense rows, then vbs::attn_stream_rt_kernel with the
// frames' nkeys live rows as keys, at either geometry
static int run_attention(const VbModel* m, const SliceView& v, const BlockW& b, const float* rstd, int B, hipStream_t st, const Err& E,
                         bool ce = false, const uint32_t* keys = nullptr, int Lp = 0, int nkeys = 0) {
    int rc;
    const int C = m->C, HEADS = m->HEADS;
    if (m->fused_qkv && !m->g384 && !ce) {
        vbq::Args qa{};
        qa.X = v.xn; qa.W = b.wqkv.p; qa.bias = b.bqkv.p; qa.rstd = rstd; qa.out = v.ao; qa.B = B; qa.heads = HEADS;
        static const int hgv = env_int("VB_QA_HGROUP", -1);      // heads walked together: the model point's, or the experiment's where it divides
        const int hg = hgv < 0 ? model_point(C)->hgroup : hgv;
        qa.hgroup = (hg > 0 && HEADS % hg == 0) ? hg : HEADS;
        dispatch_width(C, [&](auto W) {      // width 768: the non-template kernel
            constexpr int CW = decltype(W)::value;
            if constexpr (CW == C_BASE) hipLaunchKernelGGL(vbq::qkv_attn_kernel, dim3(persistent_grid(v.cus)), dim3(512), vbq::LDS_BYTES, st, qa);
            else hipLaunchKernelGGL(vbq::qkv_attn_wide_kernel<CW>, dim3(persistent_grid(v.cus)), dim3(512), vbq::LDS_BYTES, st, qa);
        });
        VB_HIP(hipGetLastError());
        return VT_OK;
    }
    const int L = Lp ? Lp : m->L, M = B * L;      // rows of a frame, of the slice
    vbg::Args a{};
    a.rstd = rstd;
    a.X = v.xn; a.W = b.wqkv.p; a.bias = b.bqkv.p; a.out = v.qk;          // q | k: rows 0 .. 2C of W_qkv
    a.M = M; a.N = 2 * C; a.K = C; a.ldo = 2 * C; a.rb = 4;    // 4 tile rows x 8 columns per XCD: measured 4 % faster than row-major
    if ((rc = launch_tile<vbg::A_PLAIN, vbg::EPI_BF16>(m, a, 1, st, E, v.cus))) return rc;
    vbg::Args w{};
    w.X = v.xn; w.W = b.wqkv.p + (size_t)2 * C * C; w.bias = b.bqkv.p + 2 * C; w.vt = v.vt;   // v: rows 2C .. 3C, stored transposed
    w.M = M; w.N = C; w.K = C; w.L = L; w.rstd = rstd;
    // (always the 256 x 256 tile: the transposed store moves 128 tokens of a feature per row, TM == 8 -- vb_gemm.h)
    if ((rc = launch_wide<vbg::A_PLAIN, vbg::EPI_VT>(w, 1, st, E, v.cus))) return rc;
    if (Lp)
        hipLaunchKernelGGL(vbs::attn_stream_rt_kernel, dim3(B * HEADS * vbs::splits_rt(Lp)), dim3(256), vbs::LDS_BYTES, st, v.qk, v.vt, v.ao, HEADS, Lp, nkeys);
    else if (keys || m->g384 || m->attn_stream || ce)
        dispatch_geo(m, [&](auto G) {
            constexpr int LG = decltype(G)::value;
            const dim3 grid(B * HEADS * vbs::splits<LG>());
            if (keys) hipLaunchKernelGGL((vbs::attn_stream_masked_kernel<LG>), grid, dim3(256), vbs::LDS_BYTES, st, v.qk, v.vt, v.ao, HEADS, keys);
            else hipLaunchKernelGGL((vbs::attn_stream_kernel<LG>), grid, dim3(256), vbs::LDS_BYTES, st, v.qk, v.vt, v.ao, HEADS);
        });
    else
        hipLaunchKernelGGL((vba::attn_kernel<L256, HD>), dim3(B * HEADS), dim3(256), (vba::Geo<L256, HD>::LDS_BYTES), st, v.qk, v.vt, v.ao, HEADS);
    VB_HIP(hipGetLastError());
    return VT_OK;
}

// Candidate elimination (vb_ce.h) along one vb::blocks call on a slice: from the first stage's block on the attention is the streaming
// kernel, under the key bitmap the stages so far have left for the slice's frames (masked form) or on the rows the last stage gathered
// (compact form); a stage runs behind its block's attention: score, then select.  A plain model: `on` is false and nothing below changes.
namespace {
struct CeWalk {
    const VbModel* const m;
    const SliceView& v;
    const int B;
    const bool on, compact;
    const uint32_t* keys = nullptr;         // masked form: the bitmap the last stage left; nullptr: every key present
    const int32_t* cidx = nullptr;          // compact form: the current index table; nullptr: nothing compacted yet
    int stage = 0, kept;                    // the next stage; the search tokens still there
    int Lc, nkeys, M;                       // rows and live rows of a frame at the current stage; the slice's residual rows, B * Lc
    const bf16* proj_x = nullptr;           // where this block's proj GEMM reads the attention rows and their centring means: v.ao and the
    const float* proj_cm = nullptr;         // caller's, or where the stage's gather left them
    CeWalk(const VbModel* m, const SliceView& v, int B)
        : m(m), v(v), B(B), on(m->ce_first >= 0), compact(on && m->ce_form == VT_CE_COMPACT), kept(m->LX), Lc(m->L), nkeys(m->L), M(B * m->L) {}

    // The score of the q | k rows the block's attention left in v.qk, into part.  Every template row (CE_TEMPLATE_RANGE ALL) takes whole query
    // tiles on the MFMA, a selection of rows (or VB_CE_SCORE_PLAIN) the plain loop.  Full frames run the <L> kernels under the key bitmap
    // `bits` (nullptr: every key); compacted frames (rt) of Lc rows, the first nkeys of them live, the run-time kernels.
    int launch_score(float* part, const uint32_t* bits, bool rt, hipStream_t st, const Err& E) const {
        const int H = m->HEADS, LZ = m->LZ, nrows = m->ce_nrows;
        const int32_t* rows = m->ce_rows.p;
        const dim3 grid(B * H);
        const bool all = nrows == LZ && !m->ce_plain;
        if (!rt)
            dispatch_geo(m, [&](auto G) {
                constexpr int L = decltype(G)::value;
                if (all) hipLaunchKernelGGL(vbc::ce_score_all_kernel<L>, grid, dim3(256), 0, st, v.qk, bits, part, H, LZ);
                else hipLaunchKernelGGL(vbc::ce_score_kernel<L>, grid, dim3(256), 0, st, v.qk, bits, rows, nrows, part, H, LZ);
            });
        else if (all) hipLaunchKernelGGL(vbc::ce_score_all_rt_kernel, grid, dim3(256), 16 * Lc * 4, st, v.qk, Lc, nkeys, part, H, LZ);
        else if (Lc <= 320) hipLaunchKernelGGL(vbc::ce_score_rt_kernel<5>, grid, dim3(256), 4 * Lc * 4, st, v.qk, Lc, nkeys, rows, nrows, part, H, LZ);
        else hipLaunchKernelGGL(vbc::ce_score_rt_kernel<12>, grid, dim3(256), 4 * Lc * 4, st, v.qk, Lc, nkeys, rows, nrows, part, H, LZ);
        VB_HIP(hipGetLastError());
        return VT_OK;
    }

    // Behind the attention of block i: the stage that sits there, if one does and it removes something (a stage that keeps every token it
    // meets is a no-op, as attn_blocks.py:40-41 returns early).  cmean: the rows' centring means while nothing has moved them.
    int after_attention(int i, const float* cmean, hipStream_t st, const Err& E) {
        proj_x = v.ao; proj_cm = cmean;
        if (!on || stage >= (int)m->ce_loc.size() || m->ce_loc[stage] != i) return VT_OK;
        const int k = stage++, keep = m->ce_keep[k];
        if (keep >= kept) return VT_OK;
        const size_t LX = (size_t)m->LX;
        float* part = m->ce_part.p + v.f0 * m->HEADS * LX;
        uint8_t* removed = m->ce_removed.p + v.f0 * LX;
        float* scores = m->ce_scores.p + ((size_t)k * m->maxB + v.f0) * LX;
        const float scale = 1.0f / (float)(m->HEADS * m->ce_nrows);
        if (int rc = launch_score(part, keys, cidx != nullptr, st, E)) return rc;
        if (int rc = compact ? compact_stage(k, part, removed, scores, scale, st, E) : masked_stage(k, part, removed, scores, scale, st, E)) return rc;
        kept = keep;
        return VT_OK;
    }

    int masked_stage(int k, const float* part, uint8_t* removed, float* scores, float scale, hipStream_t st, const Err& E) {
        uint32_t* next = m->ce_bits.p + ((size_t)k * m->maxB + v.f0) * m->ce_words();
        hipLaunchKernelGGL(vbc::ce_select_kernel, dim3(B), dim3(256), 0, st, part, keys, next, removed, scores, m->HEADS, scale, k + 1, m->ce_keep[k], m->L, m->LZ);
        VB_HIP(hipGetLastError());
        keys = next;
        return VT_OK;
    }

    // The compact form: the same score on the current rows (the first removing stage on the full frame, with the <L> kernels; later ones on
    // the compacted rows at their run-time length), select on the current candidates, then the gather of the kept rows of ao / resid (and the
    // rows' centring means) to the next stride.  The gather goes through the MLP's hidden workspace, idle between fc2 and the next fc1: frames
    // are gathered in parallel and a frame's destination overlaps earlier frames' sources.  The residual rows are copied back; the proj
    // GEMM, which follows, reads the attention rows and the means where the gather left them (proj_x / proj_cm).
    int compact_stage(int k, const float* part, uint8_t* removed, float* scores, float scale, hipStream_t st, const Err& E) {
        const int keep = m->ce_keep[k], C = m->C, Ln = m->ce_lp(k);
        const size_t LX = (size_t)m->LX, rows = (size_t)B * Ln;
        int32_t* next = m->ce_index.p + m->ce_index_off[k] + v.f0 * keep;
        int32_t* src = m->ce_src.p + v.f0 * LX;
        hipLaunchKernelGGL(vbc::ce_select_compact_kernel, dim3(B), dim3(256), 0, st, part, cidx, next, src, m->ce_inv.p + v.f0 * LX, removed, scores, m->HEADS,
                           scale, k + 1, kept, keep, m->LX);
        VB_HIP(hipGetLastError());
        bf16* gao = v.hid;
        float* gres = reinterpret_cast<float*>(v.hid + rows * C);
        float* gmean = gres + rows * C;
        hipLaunchKernelGGL(vbc::ce_gather_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, v.ao, v.resid, v.rmean, src, gao, gres, gmean, B, Lc, Ln,
                           m->LZ, keep, m->LX, C);
        VB_HIP(hipGetLastError());
        VB_HIP(hipMemcpyAsync(v.resid, gres, rows * C * 4, hipMemcpyDeviceToDevice, st));
        Lc = Ln; nkeys = m->LZ + keep; M = B * Ln; cidx = next;
        proj_x = gao;
        if (proj_cm) proj_cm = gmean;
        return VT_OK;
    }

    // Behind the last block: the final norm, whose rows of removed tokens are zeros (vit_ce.py:170-181).  Compacted rows scatter through the
    // last stage's table; dense rows take the plain norm and then the zeros under the last bitmap.
    int tail(hipStream_t st, const Err& E, float* feat_out, float* resid_out) const {
        const int C = m->C;
        const size_t LX = (size_t)m->LX;
        if (cidx) {
            const int32_t* inv = m->ce_inv.p + v.f0 * LX;
            if (resid_out) {
                hipLaunchKernelGGL(vbc::ce_scatter_rows_kernel, dim3((B * m->L + 3) / 4), dim3(256), 0, st, v.resid, inv, resid_out, B, Lc, m->L, m->LZ, C);
                VB_HIP(hipGetLastError());
            }
            hipLaunchKernelGGL(vbc::ce_final_norm_kernel<C_BASE>, dim3((B * m->LX + 3) / 4), dim3(256), 0, st, v.resid, m->ng.p, m->nb.p, LN_EPS, inv, B, Lc,
                               m->LZ, m->LX, m->F, v.map[0], feat_out);
            VB_HIP(hipGetLastError());
            return VT_OK;
        }
        if (resid_out) VB_HIP(hipMemcpyAsync(resid_out, v.resid, (size_t)M * C * 4, hipMemcpyDeviceToDevice, st));
        if (int rc = run_layernorm(m, v.resid, m->ng.p, m->nb.p, B, st, nullptr, v.map[0], feat_out, E)) return rc;
        if (keys) {
            hipLaunchKernelGGL(vbc::ce_zero_rows_kernel, dim3(grid256((size_t)B * LX * (C / 4))), dim3(256), 0, st, keys, v.map[0], feat_out, B, m->L, m->LZ, m->F, C);
            VB_HIP(hipGetLastError());
        } else if (m->ce_set)      // no stage ran in [0, nblocks) (or every stage is a no-op): nothing is removed
            VB_HIP(hipMemsetAsync(m->ce_removed.p + v.f0 * LX, 0, (size_t)B * LX, st));
        return VT_OK;
    }
};
}  // namespace

int blocks(VbModel* m, const float* tokens_in, int B, int nblocks, hipStream_t st, float* feat_out, float* resid_out, std::string* err,
           const Slice* sl) {
    const Err E{err};
    int rc = check(m, B, E);
    if (rc || (rc = check_slice(m, B, sl, E))) return rc;
    const int C = m->C, HID = m->HID;
    const SliceView v(m, B, sl);
    if (nblocks < 0 || nblocks > m->depth) nblocks = m->depth;
    if (tokens_in && tokens_in != v.resid)
        VB_HIP(hipMemcpyAsync(v.resid, tokens_in, (size_t)B * m->L * C * 4, hipMemcpyDeviceToDevice, st));
    if (m->precision == VT_PRECISION_FP32) return blocks_f32(m, B, nblocks, st, feat_out, resid_out, v, E);
    CeWalk ce(m, v, B);      // ce.M: the slice's residual rows, B frames of L; behind a compacting stage, B frames of ce.Lc
    const bool fold = m->fold;
    float* const rstd = fold ? v.rstd : nullptr;
    // folded LayerNorms: a residual stream from outside has no bf16 copy / rstd yet (vb::stem leaves both behind its GEMM)
    const float* const cmean = (fold && m->center) ? v.rmean : nullptr;
    if (fold && tokens_in && nblocks > 0 && (rc = run_layernorm(m, v.resid, nullptr, nullptr, B, st, nullptr, nullptr, nullptr, E, v.xn, rstd, v.rmean))) return rc;
    // a GEMM onto the residual stream; feeds_ln: a folded LayerNorm reads what it leaves (bf16 copy centred on cmean + statistics, then finalize)
    auto resid_gemm = [&](const bf16* X, const bf16* W, const float* bias, int K, bool feeds_ln, const float* cm) {
        vbg::Args p{};
        p.X = X; p.W = W; p.bias = bias; p.resid = v.resid; p.M = ce.M; p.N = C; p.K = K;
        if (feeds_ln) { v.stats_of(p); p.cm = cm; }
        if (int r = launch_tile<vbg::A_PLAIN, vbg::EPI_RESID>(m, p, 1, st, E, v.cus)) return r;
        return feeds_ln ? run_finalize(m, v, ce.M, st, E) : VT_OK;
    };
    for (int i = 0; i < nblocks; ++i) {
        const BlockW& b = m->blk[i];
        if (!fold && (rc = run_layernorm(m, v.resid, b.ln1g.p, b.ln1b.p, B, st, v.xn, nullptr, nullptr, E, nullptr, nullptr, nullptr, ce.M))) return rc;
        if ((rc = run_attention(m, v, b, rstd, B, st, E, ce.on && i >= m->ce_first, ce.keys, ce.cidx ? ce.Lc : 0, ce.nkeys))) return rc;
        if ((rc = ce.after_attention(i, cmean, st, E))) return rc;      // a candidate-elimination stage, where one sits behind this block
        if ((rc = resid_gemm(ce.proj_x, b.wproj.p, b.bproj.p, C, fold, ce.proj_cm))) return rc;
        if (!fold && (rc = run_layernorm(m, v.resid, b.ln2g.p, b.ln2b.p, B, st, v.xn, nullptr, nullptr, E, nullptr, nullptr, nullptr, ce.M))) return rc;
        vbg::Args f1{};
        f1.rstd = rstd;
        f1.X = v.xn; f1.W = b.w1.p; f1.bias = b.b1.p; f1.out = v.hid; f1.M = ce.M; f1.N = HID; f1.K = C; f1.ldo = HID; f1.rb = 4;
        if ((rc = launch_tile<vbg::A_PLAIN, vbg::EPI_GELU>(m, f1, 1, st, E, v.cus))) return rc;
        if ((rc = resid_gemm(v.hid, b.w2.p, b.b2.p, HID, fold && i + 1 < nblocks, cmean))) return rc;      // the final norm reads the f32 stream itself
    }
    return ce.tail(st, E, feat_out, resid_out);
}

int gemm_form(const VbModel* m, int B) {
    const int M = B * m->L, C = m->C;
    int form = 0;
    if (m->precision == VT_PRECISION_FP32) {      // the mode's launches: the qkv projection is always one GEMM of 3 C columns; conv1 of 768
        if (narrow_pick(m, B * m->LX, C, 1, 0)) form |= VT_GEMM_PATCH;
        if (narrow_pick(m, M, C, 1, 0)) form |= VT_GEMM_PROJ | VT_GEMM_FC2;
        if (narrow_pick(m, M, 3 * C, 1, 0)) form |= VT_GEMM_QK;
        if (narrow_pick(m, M, m->HID, 1, 0)) form |= VT_GEMM_FC1;
        if (narrow_pick(m, B * m->LX, 3 * HEAD_CH[1], 1, 0)) form |= VT_GEMM_HEAD;
        return form;
    }
    if (narrow_pick(m, M, C, 1, 0)) form |= VT_GEMM_PATCH | VT_GEMM_PROJ | VT_GEMM_FC2;
    // the q | k projection is a GEMM of its own only outside the fused qkv + attention kernel (run_attention)
    if ((!m->fused_qkv || m->g384 || m->ce_first >= 0) && narrow_pick(m, M, 2 * C, 1, 0)) form |= VT_GEMM_QK;
    if (narrow_pick(m, M, m->HID, 1, 0)) form |= VT_GEMM_FC1;
    if (narrow_pick(m, B * m->LX, 3 * HEAD_CH[1], 1, 0)) form |= VT_GEMM_HEAD;
    return form;
}

int head(VbModel* m, const float* feat_in, int B, hipStream_t st, float* score, float* size, float* offset, std::string* err,
         const Slice* sl) {
    const Err E{err};
    int rc = check(m, B, E);
    if (rc || (rc = check_slice(m, B, sl, E))) return rc;
    const int LX = m->LX, F = m->F, M = B * LX, C = m->C;
    const SliceView v(m, B, sl);
    if (m->precision == VT_PRECISION_FP32) return head_f32(m, feat_in, B, st, score, size, offset, v, E);
    const long long Bt = v.Bt, P2 = (long long)(F + 2) * (F + 2);              // tower-major buffers: [tower][Bt frames]...
    if (feat_in) {
        hipLaunchKernelGGL(vbm::feat_to_map_kernel, dim3(grid256((size_t)B * LX * (C / 4))), dim3(256), 0, st, feat_in, v.map[0], B, F, C);
        VB_HIP(hipGetLastError());
    }
    {   // conv1 of the three towers as one GEMM: N = 3 x 256, K = 9 x the width
        vbg::Args a{};
        a.X = v.map[0]; a.W = m->wc[0].p; a.bias = m->bc[0].p; a.out = v.map[1];
        a.M = M; a.N = 3 * HEAD_CH[1]; a.K = 9 * C; a.ldo = HEAD_CH[1]; a.C = C; a.F = F; a.out_padded = 1;
        a.n_split = HEAD_CH[1]; a.gOut = Bt * P2 * HEAD_CH[1];
        if ((rc = launch_tile<vbg::A_CONV, vbg::EPI_CONV>(m, a, 1, st, E, v.cus))) return rc;
    }
    for (int li = 1; li < 4; ++li) {   // conv2..4: one launch per layer, blockIdx.y = tower
        const int cin = HEAD_CH[li], cout = HEAD_CH[li + 1], rows = head_rows(li, cout);
        vbg::Args a{};
        a.X = v.map[li]; a.W = m->wc[li].p; a.bias = m->bc[li].p; a.out = v.map[li + 1];
        a.M = M; a.N = cout; a.K = 9 * cin; a.ldo = cout; a.C = cin; a.F = F; a.out_padded = li < 3;
        a.gX = Bt * P2 * cin; a.gW = (long long)rows * 9 * cin; a.gBias = cout;
        a.gOut = li < 3 ? Bt * P2 * cout : Bt * LX * cout;
        if (li == 1 ? (rc = launch_tile<vbg::A_CONV, vbg::EPI_CONV>(m, a, 3, st, E, v.cus))
                    : (rc = launch_gemm<256, 64, 8, 1, vbg::A_CONV, vbg::EPI_CONV>(a, 3, st, E, v.cus))) return rc;
    }
    hipLaunchKernelGGL((vbm::conv5_kernel<32>), dim3((M + 255) / 256), dim3(256), 0, st, v.map[4], m->w5.p, m->b5.p, M, LX,
                       (size_t)(Bt * LX * HEAD_CH[4]), score, size, offset);
    VB_HIP(hipGetLastError());
    return VT_OK;
}

}  // namespace vb

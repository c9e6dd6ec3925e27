/* vittrack.h -- C ABI of the MI355X-native vit_dist inference path (libvittrack_hip.so).
 *
 * Drop-in boundary for ONE hot path of lpylpy0514/VitTracker: the per-frame forward of the
 * `vit_dist` tracker.  Every entry point names the reference interface it replaces
 * (paths relative to the reference root).  Plain pointers and sizes only: no torch / Python
 * types cross this boundary.  Device pointers are HIP device addresses (fp32, contiguous);
 * `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *
 * Conventions
 *   - Every function returns 0 on success or a negative VT_ERR_* code; vt_last_error() gives a
 *     human-readable message for the calling thread (the reference raises Python exceptions,
 *     lib/test/evaluation/running.py:138-142 swallows them per sequence).
 *   - No entry point that takes a `stream` synchronises with the host or allocates memory, so all
 *     of them may be captured into a hipGraph (the reference syncs once per frame in `.tolist()`,
 *     lib/test/tracker/vit_dist.py:108-109; here the caller decides when to read results back).
 *   - A model is not thread-safe and owns ONE set of workspaces: calls on the same model must not overlap each other (issue
 *     them on one stream, or order the streams).  Independent models -- each with its own workspaces, weights replica and graphs --
 *     may run concurrently on different streams of the same GPU: two models stepped alternately on two streams are how many
 *     independent sequences are served fastest (the reference runs one tracker instance per worker process,
 *     lib/test/evaluation/running.py:105-112).
 */
#ifndef VITTRACK_H
#define VITTRACK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VT_OK 0
#define VT_ERR_ARG (-1)         /* bad argument / unsupported geometry */
#define VT_ERR_HIP (-2)         /* a HIP runtime call failed */
#define VT_ERR_STATE (-3)       /* weights not loaded, batch larger than max_batch, ... */
#define VT_ERR_MISSING_KEY (-4) /* vt_load_weights: a required tensor is absent or mis-shaped */

typedef struct vt_model vt_model;
typedef struct vt_graph vt_graph;

/* Replaces the cfg fields read by build_ostrack_dist (lib/models/vit_dist/vit_dist.py:159-164)
 * and build_box_head CENTER (lib/models/layers/head.py:352-359).
 *
 * SUPPORTED SHAPES.  The reference builds from any cfg (lib/models/vit_dist/vit_dist.py:159-198; lib/utils/ce_utils.py:22-32 lists
 * template feature sizes 8 / 12 / 7 / 14).  vt_create accepts:
 *     stride 16, depth 1..12, (template, search) = ANY multiples of 16 in [16, 512], and (round 6) ANY widths:
 *         channels a multiple of 8 (the stem's widths are C/8, C/4, C/2, C), heads dividing channels (head dimension <= 256),
 *         head_channels a multiple of 8 (the towers' widths are W, W/2, W/4, W/8)
 *     The shipped widths (channels 48, heads 1, head_channels 32) at (64, 128) and (128, 256) run the tuned kernels (every form of
 *     MFMA, LDS-resident maps, hipGraph-sized forms).  Every other geometry -- e.g. (112, 224), (192, 384); token
 *     counts need not be multiples of 16 -- and every other width -- e.g. 64 / 2 / 64 -- runs the shape-generic kernels of vt_generic.h:
 *     plain fp32, one thread per output value, reference-implementation speed, the same outputs (held to the reference's own outputs at
 *     two other width triples: tests/golden/make_golden_cfg.py) and the whole ABI (stages, template cache, graphs, vt_crop / vt_track_step,
 *     uint8 patches).
 *     channels 768, heads 12, head_channels 256, stride 16, depth 1..24 (12), (template, search) = (128, 256) or (192, 384) -- ViT-Base:
 *         OSTrack-256 (64 + 256 = 320 tokens, 16 x 16 maps) and OSTrack-384 (144 + 576 = 720 tokens, 24 x 24 maps)
 *     channels 1024, heads 16, head_channels 256, stride 16, depth 1..24 (24), the same two (template, search) pairs -- ViT-Large: the same
 *         kernels at the second width.  This exact tuple is the ViT-Large model; any other 1024-wide configuration is a shape-generic one.
 * and rejects everything else with VT_ERR_ARG and a message naming these.  vt_create_vit (below) accepts the patch-16 ViT family by name:
 *     (channels, heads) = (192, 3) ViT-Tiny, (384, 6) ViT-Small -- depth 1..12 (12), MLP 4 x channels --, (768, 12), (1024, 16) as above;
 *         head_channels 256, stride 16, (template, search) = (128, 256) or (192, 384).  Under vt_create 192 / 3 and 384 / 6 are shape-generic
 *         vit_dist models: the entry point, not the widths, names the family.
 * The tuned kernels are specialised on their tile
 * counts (token tiles per frame, feature chunks, map sides are template parameters -- that is where their register blocking comes
 * from), so widths and crop sizes are NOT run-time parameters of THOSE kernels. */
typedef struct vt_config {
    int32_t template_size; /* DATA.TEMPLATE.SIZE  (128; 64 for G128) */
    int32_t search_size;   /* DATA.SEARCH.SIZE    (256; 128 for G128) */
    int32_t channels;      /* MODEL.BACKBONE.CHANNELS (48)  */
    int32_t heads;         /* MODEL.BACKBONE.HEADS    (1)   */
    int32_t depth;         /* build_ostrack_dist(depth=3)   */
    int32_t head_channels; /* MODEL.HEAD.NUM_CHANNELS (32)  */
    int32_t stride;        /* MODEL.BACKBONE.STRIDE   (16)  */
    int32_t max_batch;     /* workspace is sized for this many frames per call */
} vt_config;

/* One named host tensor of the reference's ckpt['net'] state dict. */
typedef struct vt_tensor {
    const char* name;  /* e.g. "blocks.0.attn.qkv.weight" */
    const float* data; /* host pointer, fp32, contiguous, PyTorch layout */
    int64_t numel;
} vt_tensor;

/* Device output buffers of one forward; any pointer may be NULL (that output is then kept in
 * the model's own scratch).  Shapes follow OstrackDist.forward_head's dict
 * (lib/models/vit_dist/vit_dist.py:149-152) plus the tracker's Hann-windowed decode. */
typedef struct vt_outputs {
    float* score_map;  /* (B,1,F,F)  clamp(sigmoid)            head.py:201 */
    float* size_map;   /* (B,2,F,F)  clamp(sigmoid)            head.py:201 */
    float* offset_map; /* (B,2,F,F)  raw                       head.py:201 */
    float* pred_boxes; /* (B,4) cx,cy,w,h from the raw score   head.py:136,142-160 */
    float* hann_boxes; /* (B,4) cx,cy,w,h from hann2d*score    lib/test/tracker/vit_dist.py:104-105 */
    float* conf;       /* (B,)  max of the raw score map       lib/test/tracker/vit_dist.py:148 */
} vt_outputs;

const char* vt_last_error(void);
const char* vt_version(void);

/* build_ostrack_dist(cfg) + .cuda() on the current device (vit_dist.py:159-164;
 * lib/test/tracker/vit_dist.py:24-28).  Supported: see SUPPORTED SHAPES above (the shipped vit_48_h32 on tuned kernels -- fp32, or
 * f16 contractions in libvittrack_hip_f16.so --, any other widths / stride-16 geometry on the shape-generic fp32 kernels), and
 * channels 768, heads 12, head_channels 256 at (128,256) or (192,384): the OSTrack-256 / OSTrack-384 ViT-Base
 * (lib/models/ostrack/ostrack.py:164-286 with lib/models/ostrack/vit.py:94-139; bf16 contractions).  The two geometries run the same
 * GEMM, LayerNorm and head kernels on run-time token counts and map sides; attention is the 320-token kernels at (128,256) (fused with
 * the qkv projection unless VB_FUSED_QKV=0) and, at (192,384), always qk GEMM + v GEMM + the key-streaming kernel of vb_attn_stream.h
 * (VB_FUSED_QKV has no effect there; VB_ATTN_STREAM=1 with VB_FUSED_QKV=0 selects that kernel at (128,256) too).  Crops are 192 px /
 * 384 px, uint8 patches (B,384,384,3) with 1152-byte rows, the template cache max_batch x 144 operand rows, the Hann window 576 values.
 * Any other ViT-Base geometry or width: VT_ERR_ARG, "unsupported ViT-Base configuration" naming both.
 * channels 1024, heads 16, head_channels 256, stride 16 at the same two geometries: the ViT-Large OSTrack (vit_large_patch16_224: MLP 4096,
 * depth up to 24) on the same code with the same routes per geometry; vt_query reports channels = 1024, stage tensors are (B, L, 1024).
 * A depth outside 1..24 there: VT_ERR_ARG, "unsupported ViT-Large configuration". */
int vt_create(const vt_config* cfg, vt_model** out);
/* The patch-16 OSTrack ViT family by name (the reference's build_small_ostrack, lib/models/ostrack/ostrack.py:288-342, and its
 * vit_base / vit_large backbones): (channels, heads) = (192, 3) ViT-Tiny, (384, 6) ViT-Small -- depth 1..12, MLP 4 x channels --,
 * (768, 12), (1024, 16); head_channels 256, stride 16, (template, search) = (128, 256) or (192, 384).  For the last two tuples it is
 * vt_create.  The first two are shape-generic vit_dist models under vt_create (a different network: LeViT stem), so the family has its own
 * entry point; the model it returns is a ViT-Base-path model at that width in every respect (stage tensors (B, L, channels), vt_query
 * reports the width, vt_load_weights wants the OSTrack ckpt['net'] keys at these shapes, template cache, uint8 patches, vt_track_step*,
 * graphs, vt_gemm_form / VB_GEMM_NARROW, VB_LN_FOLD, VB_FUSED_QKV).  Kernels: the same GEMMs (an odd number of 64-deep k-tiles -- K = 192,
 * 1728 -- runs the two-buffer loop; a 64-column slice of a tile past N = 192 / 384 writes nothing), LayerNorm at 64 lanes x float2 / float
 * x 3, the fused qkv + attention kernel at 6 / 3 k-tiles.  Candidate elimination stays a width-768 feature.  Anything else: VT_ERR_ARG,
 * "unsupported ViT configuration" naming the four tuples and both geometries. */
int vt_create_vit(const vt_config* cfg, vt_model** out);
void vt_destroy(vt_model* m);

/* network.load_state_dict(ckpt['net'], strict=False) (lib/test/tracker/vit_dist.py:25):
 * unknown names (e.g. training-only convs.*) are ignored, a missing required name is an error.
 * BatchNorm is folded into the convs here exactly as Conv2d_BN.fuse does
 * (lib/models/vit_dist/vit_dist.py:22-33), weights are packed into MFMA operand images and
 * uploaded. */
int vt_load_weights(vt_model* m, const vt_tensor* tensors, int32_t n);

/* Overrides the motion window (default: hann2d(F), lib/test/utils/hann.py:6-16, computed at
 * vt_create with libm cosf, which may differ from the reference's torch float32 window by a few
 * ulps, e.g. at F = 14, 16 and 24; vittracker_amd.native.Model uploads the torch window at
 * construction).  host_window: F*F floats. */
int vt_set_window(vt_model* m, const float* host_window);

/* OstrackDist.forward(z, x) + CenterPredictor.forward + the tracker's windowed cal_bbox
 * (vit_dist.py:77-100,122-153; head.py:130-160; lib/test/tracker/vit_dist.py:103-105).
 * z_dev (B,3,Tz,Tz), x_dev (B,3,Tx,Tx) NCHW fp32 on the device.
 * z_dev may be NULL after vt_set_template: the cached template is used (same result, bit for bit). */
int vt_forward(vt_model* m, const float* z_dev, const float* x_dev, int32_t B, void* stream,
               const vt_outputs* out);

/* Exact template cache (BASELINE config 5).  The tracker stores the template crop at initialize() and feeds the SAME
 * tensor to every forward (lib/test/tracker/vit_dist.py:57-60,87-88); patch_embed(z) + pos_embed_z and block 0's
 * LayerNorm-1 + qkv of those rows are per-token functions of it (vit_dist.py:78-89), hence frame-invariant.  This
 * computes them once for B sequences and keeps them in the model; later vt_forward / vt_graph_capture calls with
 * z_dev == NULL skip that work.  Deeper layers are NOT cached: from block 0's attention on, template tokens depend on
 * the current search tokens.
 * ViT-Base: what is cached is the templates' bf16 patch-GEMM operand rows (the fp32 -> bf16 gather of z); every step that reads the
 * cache -- and every vt_forward_u8 with a template of its own -- embeds template rows and search rows with two GEMMs on dense operands,
 * so cache on == cache off bit for bit, eager and captured (captured steps of >= 64 frames keep their two chains with z_dev == NULL). */
int vt_set_template(vt_model* m, const float* z_dev, int32_t B, void* stream);

/* --- the three stages of vt_forward, individually (parity tests, profiling) ----------------- */
/* patch_embed(z), patch_embed(x), += pos_embed, cat (vit_dist.py:78-84) -> tokens (B,L,C). */
int vt_stem(vt_model* m, const float* z_dev, const float* x_dev, int32_t B, void* stream,
            float* tokens_dev);
/* blocks[0..nblocks) then self.norm (vit_dist.py:88-94).  nblocks<0 = all.  feat_dev (B,Lx,C) =
 * normalised search tokens (the head's input, vit_dist.py:126); resid_dev (B,L,C), optional =
 * the un-normalised residual stream after the last executed block. */
int vt_blocks(vt_model* m, const float* tokens_dev, int32_t B, int32_t nblocks, void* stream,
              float* feat_dev, float* resid_dev);
/* forward_head + CenterPredictor (vit_dist.py:122-153; head.py:130-201) on (B,Lx,C) tokens. */
int vt_head(vt_model* m, const float* feat_dev, int32_t B, void* stream, const vt_outputs* out);

/* box_head.cal_bbox(score, size, offset, return_score=True) (head.py:142-160) on arbitrary
 * device maps: bbox_dev (B,4), max_score_dev (B,) optional. First maximum wins ties. */
int vt_cal_bbox(vt_model* m, const float* score_dev, const float* size_dev, const float* offset_dev,
                int32_t B, void* stream, float* bbox_dev, float* max_score_dev);

/* --- the steps either side of the network in track(), on the device ---- */
/* sample_target(image, state, factor, output_sz) + Preprocessor.process
 * (lib/train/data/processing_utils.py:12-79; lib/test/tracker/data_utils.py:11-17) for B sequences:
 * frames_dev (B,H,W,3) uint8, states_dev (B,4) double [x,y,w,h] -> crops_dev (B,3,T,T) fp32
 * normalised with mean3/std3 (host, 3 floats each) and resize_factor_dev (B) double = T / crop_sz.
 * Crop geometry in double with Python's round-half-even; resize = OpenCV INTER_LINEAR uint8
 * fixed-point scheme. */
int vt_crop(vt_model* m, const uint8_t* frames_dev, int32_t H, int32_t W, const double* states_dev, double factor,
            int32_t out_size, const float* mean3, const float* std3, int32_t B, void* stream, float* crops_dev,
            double* resize_factor_dev);
/* sample_target ALONE (lib/train/data/processing_utils.py:12-79): patch_dev (B,T,T,3) uint8 is the array sample_target returns --
 * HWC, before Preprocessor.process -- byte for byte (same geometry and fixed-point resize as vt_crop); resize_factor_dev as vt_crop.
 * A too-small box (processing_utils.py:33-34 raises) writes zeros and a NaN resize factor.
 * Every uint8 patch pointer of this header (patch_dev of vt_crop_u8 / _frames / _images, x_patch_dev of vt_stem_u8 / vt_forward_u8, and
 * crops_dev of the tracker steps, which holds the patch) must be 4-byte aligned: the kernels move a patch as 12-byte groups of four
 * pixels.  VT_ERR_ARG otherwise (ViT-Base: 16 bytes, see vt_forward_u8). */
int vt_crop_u8(vt_model* m, const uint8_t* frames_dev, int32_t H, int32_t W, const double* states_dev, double factor,
               int32_t out_size, int32_t B, void* stream, uint8_t* patch_dev, double* resize_factor_dev);
/* Preprocessor.__init__'s mean / std (lib/test/tracker/data_utils.py:8-9) for the uint8 entry points below (default: the ImageNet
 * values the reference hard-codes).  Preprocessor.process is affine per channel and the stem's first conv is linear, so the
 * normalisation is folded into that layer's weights in fp64 (here and at vt_load_weights); the conv's zero padding becomes the
 * byte value that normalises to zero.  Synchronises the device; not capturable; VT_ERR_STATE once graphs have been captured.
 * ViT-Base: folded into a second bf16 image of the patch-embedding weights that meets the CENTRED bytes p - 128:
 * W' = W / (255 std_c), b' = b - sum W mean_c / std_c + 128 sum W' from the unrounded fp64 W' (uncentred, the rounding of W' multiplies
 * the patch's common mode and the tokens leave their 3.2e-3 bound; VB_U8_CENTER=0 restores that form to show it). */
int vt_set_normalization(vt_model* m, const float* mean3, const float* std3);
/* OSTrack candidate elimination (MODEL.BACKBONE.TYPE vit_base_patch16_224_ce: lib/models/ostrack/vit_ce.py:151-186,
 * lib/models/layers/attn_blocks.py:20-85) on a ViT-Base model, by KEY MASKING: after the attention of block loc[k] the search tokens are
 * ranked by the attention they receive from the selected template rows (mean over heads and rows of the softmax weights) and the
 * stage keeps ceil(keep_ratio[k] * kept so far) of them, the product in double as math.ceil(keep_ratio * lens_s) takes it (0.7, 0.7, 0.7:
 * 180 / 126 / 89 of 256, 404 / 283 / 199 of 576).  No token is moved: every matrix keeps its B x L rows, later attentions treat the removed
 * tokens as absent keys, and the search rows of removed tokens are exact zeros after the final norm (feat_dev of vt_blocks, the head's
 * input), as in the reference.  The kept tokens' values are the reference's; there is no speed-up.
 *   n, loc, keep_ratio: 1 <= n <= depth stages, loc strictly increasing in [0, depth), 0 < keep_ratio <= 1 (host arrays)
 *   template_rows: Lz host bytes, non-zero = the template row takes part in the score (CE_TEMPLATE_RANGE: lib/utils/ce_utils.py:15-49), at
 *       least one set; NULL = all rows.  One selection per model, not per frame.
 * A stage whose count equals the previous stage's is a no-op; a configuration of no-ops only leaves the model a plain one, bit for bit.
 * Ties in the ranking go to the lower token index (the reference's torch.sort leaves them unspecified).
 * From block loc[0] on attention runs as qk GEMM + v GEMM + the key-streaming kernel at both geometries (the score reads the q | k rows).
 * Call it before or after vt_load_weights, before any graph is captured: VT_ERR_STATE afterwards, as vt_set_normalization.  Anything but a
 * ViT-Base model, or arguments outside the above: VT_ERR_ARG.  Synchronises the device and allocates; not capturable.
 * With nblocks < depth vt_blocks runs the stages inside [0, nblocks) and the final norm zeroes what they removed.  resid_dev rows of
 * removed tokens are unspecified (finite in practice: they go on being computed and are never read by a kept row). */
int vt_set_candidate_elimination(vt_model* m, int32_t n, const int32_t* loc, const double* keep_ratio, const uint8_t* template_rows);
/* The form the stages run in.  VT_CE_MASKED (the default): key masking, as above.  VT_CE_COMPACT: behind every stage the kept tokens of a
 * frame (template rows first, kept search tokens in ascending global index, zero pad rows up to a multiple of 16) are gathered into a
 * shorter dense sequence and every kernel behind it runs on B x Lp_k rows (0.7, 0.7, 0.7: 256 / 192 / 160 rows of 320, 560 / 432 / 352 of
 * 720); the final norm scatters the kept rows back to their global positions, removed rows are exact zeros, and resid_dev of vt_blocks is
 * the dense (B,L,C) stream with zero rows for removed tokens.  Same function, same vt_ce_result (global indices), same tie rule; the first
 * removing stage selects exactly as the masked form does.  ViT-Base only (VT_ERR_ARG otherwise, and for any other `form`); before or after
 * vt_set_candidate_elimination, before any graph is captured (VT_ERR_STATE afterwards).  Neither synchronises nor allocates. */
#define VT_CE_MASKED 0
#define VT_CE_COMPACT 1
int vt_set_ce_form(vt_model* m, int32_t form);
/* What the last vt_forward* / vt_track_step* / vt_blocks / graph launch of B frames left: removed_stage_dev (B,Lx) bytes, 0 = kept to the
 * end, k = removed at stage k (1-based); scores_dev (n,B,Lx) fp32, the ranking score of each stage, NaN for tokens removed earlier and for
 * stages that did not run (no-ops; stages at or past nblocks keep what an earlier call left).  Either pointer may be NULL.  Capturable.
 * VT_ERR_STATE before vt_set_candidate_elimination. */
int vt_ce_result(vt_model* m, int32_t B, void* stream, uint8_t* removed_stage_dev, float* scores_dev);
/* Preprocessor.process + OstrackDist.forward on a uint8 search patch (lib/test/tracker/data_utils.py:11-17 +
 * lib/models/vit_dist/vit_dist.py:77-100): x_patch_dev (B,S,S,3) uint8 as vt_crop_u8 writes it; z_dev (B,3,Tz,Tz) fp32 as in
 * vt_forward, or NULL after vt_set_template.  Results agree with vt_forward on the normalised fp32 crop to fp32 rounding (the
 * reference rounds three times per input value, the folded layer once; tests: maps within 1e-5), not bit for bit.
 * vit_48 path: every stem form of the tuned geometries; the shape-generic kernels normalise per tap with the reference's own three
 * rounded operations and are bit-identical to vt_forward; VT_ERR_STATE under the diagnostic switches (vt_patch_u8_supported).
 * ViT-Base: every batch size; the patch is gathered straight into the bf16 GEMM operand (exact) and the search rows agree with the
 * fp32 route to bf16 rounding of the weights (tokens within 3.2e-3 of the reference, relative to the centred rows); x_patch_dev must be
 * 16-byte aligned there (VT_ERR_ARG otherwise). */
int vt_forward_u8(vt_model* m, const float* z_dev, const uint8_t* x_patch_dev, int32_t B, void* stream, const vt_outputs* out);
/* The search rows of vt_stem from a uint8 patch: tokens_dev (B,L,C), rows [len_z, L) written, template rows untouched. */
int vt_stem_u8(vt_model* m, const uint8_t* x_patch_dev, int32_t B, void* stream, float* tokens_dev);
/* 1 when a batch of B runs a stem form that reads uint8 patches (every vit_48 form outside the diagnostic builds; ViT-Base: always), else 0. */
int vt_patch_u8_supported(const vt_model* m, int32_t B);
/* Which crop kernel form the current device runs (decided once per device by a self test against a byte-load twin):
 * 1 = the 8-byte unaligned-window form, 2 = the byte-load form, negative = the self test could not run. */
int vt_crop_form(void);
/* Which GEMM kinds of a plain vt_forward of B frames run on the narrow 128 x 64 tile instead of the 256 x 256 one (ViT-Base / ViT-Large
 * models).  Both tiles sum every output element in one workgroup in the same order, so the results are the same bits; the narrow tile is
 * chosen per launch where the wide tiles would leave most compute units idle (small B).  VB_GEMM_NARROW, read at vt_create: -1 = that
 * automatic choice (default), 0 = never, 1 = wherever a narrow instantiation exists.  A captured graph keeps the tiles of its capture.
 * The v projection (stored transposed) and head convs 2-4 of 64 columns have one tile form and no bit.  vit_48 and shape-generic models: 0.
 * NULL model: -1, vt_last_error "null model". */
#define VT_GEMM_PATCH 1  /* patch embedding */
#define VT_GEMM_QK 2     /* q | k projection, where the model's attention route launches it as a GEMM (192 / 384 geometry, candidate
                            elimination, VB_FUSED_QKV=0); 0 under the fused qkv + attention kernel */
#define VT_GEMM_PROJ 4   /* attention output projection */
#define VT_GEMM_FC1 8    /* MLP fc1 */
#define VT_GEMM_FC2 16   /* MLP fc2 */
#define VT_GEMM_HEAD 32  /* head conv1 of the three towers (and conv2, chosen by its own tile count) */
int vt_gemm_form(const vt_model* m, int32_t B);
/* The arithmetic of a patch-16 ViT model (vt_create_vit, or the ViT-Base / ViT-Large tuples of vt_create; anything else: VT_ERR_ARG).
 * VT_PRECISION_BF16 (the default): single-piece bf16 operands.  VT_PRECISION_FP32: every contraction multiplies the exact three-piece bf16
 * splits of its fp32 operands (six terms, fp32 accumulator) at six times the GEMM depth, activations between kernels are fp32, the
 * attention and GELU run in fp32: results agree with the reference's fp32 outputs to a few 1e-6 on maps.  Every entry point
 * of the model works in either mode; vt_gemm_form reports the tiles of the mode's launches (VT_GEMM_QK: the qkv projection, always a GEMM
 * there); VB_LN_FOLD and VB_FUSED_QKV have no effect in fp32 mode.  Callable before or after vt_load_weights: the weights' piece images are
 * built at whichever comes second (vt_load_weights keeps the unfolded fp32 tensors of a patch-16 ViT model in host memory for that: the model's
 * size once more, in either mode).  The mode's workspaces (the largest: max_batch x L x 4 C x 12 bytes) are allocated when it is first selected; a failed allocation leaves the model in bf16 mode (VT_ERR_HIP, the size in the message).  The mode and
 * candidate elimination exclude each other (VT_ERR_STATE from either call).  Switching drops the template cache.  Synchronises the device;
 * VT_ERR_STATE while a captured graph of the model is alive.  VB_PRECISION=fp32, read at vt_create, selects the mode from the start. */
#define VT_PRECISION_BF16 0
#define VT_PRECISION_FP32 1
int vt_set_precision(vt_model* m, int32_t precision);
/* The mode of a patch-16 ViT model.  Any other model: -1 (it has no mode; vt_last_error is left as it is).  NULL: -1, "null model". */
int vt_precision(const vt_model* m);

/* The tail of Vit_dist.track (lib/test/tracker/vit_dist.py:107-111,150-156; clip_box,
 * lib/utils/box_ops.py:97-106): scale the windowed box back to image pixels, map it to the frame,
 * clip with `margin`, and overwrite states_dev (B,4) double in place.  No host sync: a sequence can
 * run as back-to-back graph replays with its state on the device. */
int vt_update_state(vt_model* m, const float* hann_boxes_dev, const double* resize_factor_dev, int32_t search_size,
                    int32_t H, int32_t W, int32_t margin, int32_t B, void* stream, double* states_dev);
/* The same, and what `track()` returns ({"target_bbox", "confidence"}, lib/test/tracker/vit_dist.py:146-148) written as a (B,5)
 * double record [x, y, w, h, max score] to `record`: device memory, or device-mapped pinned host memory -- then the frame step
 * ends without a copy kernel or a device -> host copy, the host reads the record after one stream synchronisation.
 * conf_dev may be NULL (confidence 0). */
int vt_update_state_record(vt_model* m, const float* hann_boxes_dev, const float* conf_dev, const double* resize_factor_dev,
                           int32_t search_size, int32_t H, int32_t W, int32_t margin, int32_t B, void* stream, double* states_dev,
                           double* record);

/* The whole per-frame step of Vit_dist.track() (lib/test/tracker/vit_dist.py:87-148) in ONE call: the crop of the search region
 * (search_size of the model's config; crops_dev = a (B,3,S,S) float workspace of the caller) -> the network on the cached
 * template (vt_set_template first) -> vt_update_state_record; with the small-batch head form the decode kernel runs the tail
 * itself (one launch less per step).  record may be NULL.
 * ViT-Base: the same contract (crops_dev 16-byte aligned); from 64 frames up the network and each half's tail run as two chains over
 * frame slices, forked off `stream` after the crop and joined back with events (legal under stream capture and in eager mode;
 * VT_GRAPH_CHAINS as for vt_graph_capture), bit-identical to one chain.
 * Round 6: the crop reaches the stem as sample_target's uint8 patch -- the step is vt_crop_u8 -> vt_forward_u8(z = NULL) ->
 * vt_update_state_record, bit for bit, and crops_dev holds the (B,S,S,3) uint8 patch in its first bytes -- whenever
 * (mean3, std3) equal the model's normalisation (vt_set_normalization) and vt_patch_u8_supported(m, B); otherwise (and with
 * VT_TRACK_U8=0 in the environment at vt_create) it is vt_crop -> vt_forward(z = NULL) -> vt_update_state_record with the fp32 crop. */
int vt_track_step(vt_model* m, const uint8_t* frames, int32_t H, int32_t W, double* states_dev, double factor, const float* mean3,
                  const float* std3, int32_t B, void* stream, float* crops_dev, double* resize_factor_dev, const vt_outputs* out,
                  int32_t margin, double* record);
/* Open loop (on != 0): later vt_track_step calls -- and graphs captured from then on -- crop around states_dev, write the step's
 * box and confidence to `record`, and leave states_dev as it is: every frame is searched around boxes the CALLER provides (the
 * ground truth of an accuracy study; the held 30-90 px boxes of bench.py's tracker-step figures, which synthetic noise frames would
 * otherwise drive to the clip limits within a few frames).  The reference's track() is the closed loop (lib/test/tracker/
 * vit_dist.py:107-111 overwrites self.state), which stays the default; vt_update_state[_record] are not affected. */
int vt_set_open_loop(vt_model* m, int32_t on);

/* --- batches of frames of different sizes: one descriptor per sequence -------------------------------------------------------
 * The reference runs one tracker per sequence and worker process (lib/test/evaluation/running.py:105-112), so every sequence brings
 * its own frame size.  The dense entry points above take ONE (B,H,W,3) buffer with ONE H, W; the *_frames twins below take a (B,)
 * table of descriptors instead, in device memory or device-mapped pinned host memory.  The kernels read the table when they run: a
 * graph captured on it stays valid when the caller rewrites its contents (pointers, sizes) between replays.
 *   data:  HWC uint8, device memory or device-mapped pinned host memory, 4-byte aligned
 *   pitch: bytes between rows, >= 3*W (0 = 3*W); the frame is [data, data + pitch*(H-1) + 3*W), nothing outside it is read
 * A descriptor with a null `data`, H or W < 1, a misaligned `data` or pitch < 3*W is treated as a too-small box (processing_utils.py:
 * 33-34 raises): NaN resize factor, zero (uint8) or NaN (fp32) patch, nothing read through it; the other sequences are unaffected. */
typedef struct vt_frame {
    const uint8_t* data;
    int32_t H, W;
    int64_t pitch;
} vt_frame;

/* vt_crop with a frame table: sample_target(image_b, state_b, factor, output_sz) + Preprocessor.process per sequence
 * (lib/train/data/processing_utils.py:12-79; lib/test/tracker/data_utils.py:11-17), each sequence b on frames_dev[b] with its own
 * H, W and pitch.  Results equal vt_crop of that frame alone (B = 1), bit for bit. */
int vt_crop_frames(vt_model* m, const vt_frame* frames_dev, const double* states_dev, double factor, int32_t out_size,
                   const float* mean3, const float* std3, int32_t B, void* stream, float* crops_dev, double* resize_factor_dev);
/* vt_crop_u8 with a frame table (sample_target alone, processing_utils.py:12-79): as vt_crop_frames, the uint8 (B,T,T,3) patch. */
int vt_crop_u8_frames(vt_model* m, const vt_frame* frames_dev, const double* states_dev, double factor, int32_t out_size, int32_t B,
                      void* stream, uint8_t* patch_dev, double* resize_factor_dev);
/* vt_track_step with a frame table (lib/test/tracker/vit_dist.py:87-148 per sequence, one tracker per sequence as
 * lib/test/evaluation/running.py:105-112 runs them): the crop of vt_crop[_u8]_frames, the network on the cached template, and the
 * tail with clip_box (lib/utils/box_ops.py:97-106) against frames_dev[b].H / W of each sequence.  Same routes (uint8 patch / fp32
 * crop), open loop and models as vt_track_step; a batch of equal frames gives vt_track_step's records bit for bit. */
int vt_track_step_frames(vt_model* m, const vt_frame* frames_dev, double* states_dev, double factor, const float* mean3,
                         const float* std3, int32_t B, void* stream, float* crops_dev, double* resize_factor_dev, const vt_outputs* out,
                         int32_t margin, double* record);
/* --- frames in the pixel formats decoders and capture pipelines hand out: one vt_image descriptor per sequence ---------------
 * Each descriptor denotes one H x W 8-bit RGB image rgb(d); vt_crop_images, vt_crop_u8_images and vt_track_step_images give, bit for
 * bit, what their *_frames twins give on a tight vt_frame holding rgb(d).  Only the fetch of a source pixel differs: every bilinear
 * tap pixel is converted to RGB first, then the crop's arithmetic runs unchanged.
 *   format     planes                                          rgb(d) at pixel (x, y)
 *   RGB        plane0: H rows of 3 W bytes                     bytes 0, 1, 2 of the pixel (as vt_frame)
 *   BGR        plane0: H rows of 3 W bytes                     bytes 2, 1, 0 (cv.cvtColor(f, cv.COLOR_BGR2RGB))
 *   RGBA       plane0: H rows of 4 W bytes                     bytes 0, 1, 2; the 4th byte is never used
 *   BGRA       plane0: H rows of 4 W bytes                     bytes 2, 1, 0; the 4th byte is never used
 *   NV12/NV21  plane0: H rows of W luma bytes; plane1: H/2     BT.601 limited range, each 2 x 2 block sharing one chroma pair (no
 *              rows of W/2 byte pairs, (U,V) for NV12 and      chroma interpolation), in the fixed-point arithmetic of OpenCV's
 *              (V,U) for NV21; H and W even                    cv.cvtColor(f, cv.COLOR_YUV2RGB_NV12 / _NV21), int32, >> arithmetic:
 *       Y = luma[y][x];  U, V = chroma pair at row y >> 1, pair x >> 1;  yy = max(Y - 16, 0) * 1220542
 *       R = clamp((yy + 1673527 (V - 128)                  + (1 << 19)) >> 20, 0, 255)
 *       G = clamp((yy -  852492 (V - 128) - 409993 (U - 128) + (1 << 19)) >> 20, 0, 255)
 *       B = clamp((yy + 2116026 (U - 128)                  + (1 << 19)) >> 20, 0, 255)
 *     (1.164, 1.596, 0.813, 0.391 and 2.018 times 2^20, written down from OpenCV's ITUR_BT_601_* constants; a GPU test compares them
 *     with cv2.cvtColor where cv2 is installed.)
 *   I420/YV12  plane0: H rows of W luma bytes; plane1: the first chroma plane (U for I420, V for YV12), H/2 rows of W/2 bytes at
 *              pitch1 (0 = W/2); the second chroma plane begins pitch1 * H/2 bytes after plane1 -- the contiguous buffer of OpenCV
 *              (COLOR_YUV2RGB_I420) and av_image_copy_to_buffer.  H and W even; plane1's extent covers both chroma planes
 *              (pitch1 (H - 1) + W/2 bytes); only plane0 and plane1 need 4-byte alignment.
 *   YUYV/UYVY  plane0: H rows of 2 W bytes, each 4 bytes Y0 U Y1 V (YUYV = YUY2) or U Y0 V Y1 (UYVY): the pair shares its chroma.  W even.
 *   P010       NV12 in little-endian 16-bit samples: plane0 H rows of 2 W bytes, plane1 H/2 rows of 2 W bytes ((U, V) pairs).  The
 *              8-bit sample is the HIGH byte of each word, so a P016 surface is read the same way.  H and W even.
 *   GRAY8      plane0: H rows of W bytes; rgb = (Y, Y, Y), no conversion.
 *   RGBP/BGRP  planar RGB, three planes of H rows of W bytes: plane0 is the R plane (BGRP: the B plane) at pitch0; plane1 is the G plane
 *              at pitch1 (0 = W); the third plane (B; BGRP: R) begins pitch1 * H bytes after plane1 -- the I420 rule for a trailing
 *              plane.  rgb = (R[y][x], G[y][x], B[y][x]), no conversion.  A contiguous (3, H, W) uint8 tensor at p (torchvision's
 *              read_image / decode_jpeg, every CHW dataloader) is plane0 = p, plane1 = p + H W, pitches 0.  H and W may be odd.
 *   I444       planar 4:4:4 (ffmpeg's yuv444p): plane0 H rows of W luma bytes; plane1 the U plane, H rows of W bytes at pitch1 (0 = W);
 *              the V plane begins pitch1 * H bytes after plane1.  Every pixel has its own chroma: U, V at (x, y).  H and W may be odd.
 *   I422       planar 4:2:2 (yuv422p): as I444 with chroma planes of H rows of W/2 bytes (pitch1 0 = W/2): U, V at (x >> 1, y).  W even,
 *              H may be odd.
 *     The four planar layouts are read as single bytes: plane0 and plane1 need NO alignment (p + H W of an odd-sized CHW frame is not
 *     4-byte aligned).  plane1's extent covers both trailing planes: pitch1 (2 H - 1) + its row bytes, inside a 32-bit offset.
 * The format word: bits 0-7 the layout (the VT_PIX_* values; 6, 7, 14, 15, 20, 27-31, 35, 39, 43 and 47 up are never assigned), bits 8-11 the matrix (0 = BT.601, 1 =
 * BT.709), bits 12-15 the range (0 = limited, 1 = full), bits 16-31 zero -- format = VT_PIX_P010 | VT_PIX_BT709 | VT_PIX_FULL.  Every
 * value that was legal before the colour fields existed means what it meant (NV12 = BT.601 limited).  Matrix and range belong to the
 * YUV layouts (NV12 / NV21, I420 / YV12, YUYV / UYVY, P010, I444 / I422, YV16 / YV24, NV16 / NV24, P210 / P410, I010 ... I416); on the RGB
 * family (RGBP / BGRP included), GRAY8 and GRAY10 / GRAY12 / GRAY16 they must be 0.
 * Colour, every YUV layout: chroma is never interpolated (a 2 x 2 block of 4:2:0, a pair of 4:2:2, shares its U, V); int32, >> arithmetic:
 *       yy = max(Y - 16, 0) * cy   (limited range)      yy = Y * cy   (full range)
 *       R = clamp((yy + cvr (V - 128)                   + (1 << 19)) >> 20, 0, 255)
 *       G = clamp((yy - cvg (V - 128) - cug (U - 128)   + (1 << 19)) >> 20, 0, 255)
 *       B = clamp((yy + cub (U - 128)                   + (1 << 19)) >> 20, 0, 255)
 *       matrix, range       cy        cvr       cvg      cug      cub
 *       601 limited         1220542   1673527   852492   409993   2116026     (OpenCV's literals, as above)
 *       601 full            1048576   1470104   748826   360853   1858077
 *       709 limited         1220945   1879825   558796   223607   2215014
 *       709 full            1048576   1651297   490864   196424   1945738
 *     The three other rows are round(x 2^20) of the exact rationals: luma scale 255/219 (limited) or 1 (full); chroma scale 255/224
 *     or 1 on 2(1-Kr), 2(1-Kr)Kr/Kg, 2(1-Kb)Kb/Kg, 2(1-Kb) with Kr / Kb = 0.299 / 0.114 (BT.601) and 0.2126 / 0.0722 (BT.709).
 *     Checked on the CPU over all 2^24 (Y, U, V): the value before the shift stays below 5.8e8 (inside int32), and before clamping
 *     each channel differs from the fp64 formula by at most 0.5000 / 0.5002 / 0.5000 (601 full / 709 limited / 709 full; OpenCV's
 *     601-limited literals: up to 0.69).  tests/test_frame_formats_yuv.py repeats the check.
 *   YV16/YV24  I422 / I444 with the V plane first: plane1 is the V plane, the U plane begins pitch1 * H bytes after it.
 *   NV16       two-plane 4:2:2 (capture cards): plane0 H rows of W luma bytes; plane1 H rows of W/2 (U, V) byte pairs (pitch1 0 = W): U, V
 *              at pair x >> 1 of row y.  W even, H may be odd.
 *   NV24       two-plane 4:4:4: plane1 H rows of W (U, V) pairs, 2 W bytes (pitch1 0 = 2 W): U, V at (x, y).  H and W may be odd.
 *   P210/P410  NV16 / NV24 in little-endian 16-bit words, MSB-aligned (hardware decoders): plane0 H rows of 2 W bytes, plane1 H rows of
 *              2 W (P210) / 4 W (P410) bytes.  The 8-bit sample is the HIGH byte of each word, P010's rule: a P216 / P416 surface is read
 *              the same way.  P210: W even.
 *   16-bit planar layouts, LSB-aligned little-endian words (ffmpeg's yuv420p10le ... yuv444p16le, gray10le ... gray16le): the code is
 *              32 | sub << 2 | dep -- sub 0 / 1 / 2 / 3 = 4:2:0 / 4:2:2 / 4:4:4 / luma only, dep 0 / 1 / 2 = 10 / 12 / 16 bits:
 *              I010 / I012 / I016 = 32 / 33 / 34, I210 / I212 / I216 = 36 / 37 / 38, I410 / I412 / I416 = 40 / 41 / 42, GRAY10 / GRAY12 /
 *              GRAY16 = 44 / 45 / 46.  Planes are those of I420, I422, I444 and GRAY8 with row bytes doubled: plane0 H rows of 2 W bytes;
 *              plane1 the U plane, rows of W (4:2:0, 4:2:2) or 2 W (4:4:4) bytes; the V plane begins pitch1 * (chroma rows: H/2 for
 *              4:2:0, else H) bytes after plane1, and plane1's extent covers both.  Parity as the 8-bit layouts: H and W even for 4:2:0,
 *              W even for 4:2:2.
 *     The 8-bit sample of every 16-bit layout is s8 = min(v >> (depth - 8), 255): the top eight bits of the depth, truncated as P010's
 *     are; a word above the depth's range saturates.  Everything after s8 -- the colour rows, no chroma interpolation -- is as above.
 *     Alignment: the byte layouts (YV16 / YV24, NV16 / NV24), the high-byte ones (P210 / P410) and the 16-bit depth are read as single
 *     bytes and need none; the 10- and 12-bit layouts are fetched as 16-bit words: plane0, plane1 and both pitches must be even.
 *   Not supported: chroma interpolation and chroma siting, BT.2020 / PQ / HLG, big-endian samples.
 *   pitch0 / pitch1: bytes between rows of plane0 / plane1, >= the row's bytes (0 = the row's bytes).  A plane is [plane, plane +
 *   pitch (rows - 1) + row bytes); nothing outside it is read.  plane1 / pitch1 are unused by the one-plane formats.
 * Planes: device memory or device-mapped pinned host memory.  The table (B,) lives there too and is read when the kernels run: a
 * graph captured on it stays valid when its contents -- pointers, sizes, formats -- change between replays.  A table may mix formats.
 * A descriptor is unusable -- treated as a too-small box: NaN resize factor, zero (uint8) or NaN (fp32) patch, nothing read through
 * it, the other sequences unaffected -- when its format word is not one described above (an unassigned layout, a matrix or range
 * beyond 1, a bit in 16-31, matrix or range bits on an RGB layout or GRAY8) or `reserved` is not 0, a plane it needs is null or not
 * 4-byte aligned (the four planar layouts and codes 21-46: null only; the 10- and 12-bit layouts: null, an odd address or an odd pitch), a
 * pitch is below the row's bytes (doubled for 16-bit samples), H or W is < 1, W is odd for a 4:2:2 layout (I422, YV16, NV16, P210 and
 * I210 / I212 / I216 included), H or W is odd for a 4:2:0 layout (I010 / I012 / I016 included), or a plane does not fit a 32-bit offset. */
enum { VT_PIX_RGB = 0, VT_PIX_BGR = 1, VT_PIX_RGBA = 2, VT_PIX_BGRA = 3, VT_PIX_NV12 = 4, VT_PIX_NV21 = 5 };
/* the layouts added to bits 0-7 (6 and 7 are never assigned) ... */
#define VT_PIX_I420 8
#define VT_PIX_YV12 9
#define VT_PIX_YUYV 10
#define VT_PIX_UYVY 11
#define VT_PIX_P010 12
#define VT_PIX_GRAY8 13
/* ... the planar layouts (14 and 15 are never assigned) ... */
#define VT_PIX_RGBP 16
#define VT_PIX_BGRP 17
#define VT_PIX_I444 18
#define VT_PIX_I422 19
/* ... the V-first planar and the two-plane layouts of 4:2:2 and 4:4:4 in bytes, the two-plane ones in MSB-aligned 16-bit words (20 and
 * 27-31 are never assigned) ... */
#define VT_PIX_YV16 21
#define VT_PIX_YV24 22
#define VT_PIX_NV16 23
#define VT_PIX_NV24 24
#define VT_PIX_P210 25
#define VT_PIX_P410 26
/* ... the planar layouts in LSB-aligned little-endian 16-bit words, 32 | sub << 2 | dep: sub 0 / 1 / 2 / 3 = 4:2:0 / 4:2:2 / 4:4:4 /
 * luma only, dep 0 / 1 / 2 = 10 / 12 / 16 bits (dep 3, i.e. 35, 39, 43 and 47, and everything above 47 are never assigned) ... */
#define VT_PIX_WIDE(sub, dep) (32 | (sub) << 2 | (dep))
#define VT_PIX_I010 32
#define VT_PIX_I012 33
#define VT_PIX_I016 34
#define VT_PIX_I210 36
#define VT_PIX_I212 37
#define VT_PIX_I216 38
#define VT_PIX_I410 40
#define VT_PIX_I412 41
#define VT_PIX_I416 42
#define VT_PIX_GRAY10 44
#define VT_PIX_GRAY12 45
#define VT_PIX_GRAY16 46
/* ... and the colour tags of a YUV layout, or-ed into the format word: matrix in bits 8-11, range in bits 12-15 */
#define VT_PIX_BT601 0x0000
#define VT_PIX_BT709 0x0100
#define VT_PIX_LIMITED 0x0000
#define VT_PIX_FULL 0x1000
#define VT_PIX_LAYOUT(format) ((format) & 0xff)
typedef struct vt_image {
    const uint8_t* plane0;
    const uint8_t* plane1;
    int64_t pitch0, pitch1;
    int32_t H, W, format, reserved;
} vt_image;

/* vt_crop_frames on a (B,) vt_image table. */
int vt_crop_images(vt_model* m, const vt_image* images_dev, const double* states_dev, double factor, int32_t out_size,
                   const float* mean3, const float* std3, int32_t B, void* stream, float* crops_dev, double* resize_factor_dev);
/* vt_crop_u8_frames on a (B,) vt_image table. */
int vt_crop_u8_images(vt_model* m, const vt_image* images_dev, const double* states_dev, double factor, int32_t out_size, int32_t B,
                      void* stream, uint8_t* patch_dev, double* resize_factor_dev);
/* vt_track_step_frames on a (B,) vt_image table: the same routes, models and open loop; the tail clips each sequence against
 * images_dev[b].H / W. */
int vt_track_step_images(vt_model* m, const vt_image* images_dev, double* states_dev, double factor, const float* mean3,
                         const float* std3, int32_t B, void* stream, float* crops_dev, double* resize_factor_dev, const vt_outputs* out,
                         int32_t margin, double* record);
/* Restart single sequences (Vit_dist.initialize, lib/test/tracker/vit_dist.py:52-65, for slots whose sequence ended while the
 * others go on): rewrite the template cache rows of slots[0..n) from z_dev (n,3,Tz,Tz), under the form batch the cache was written
 * with -- afterwards a slot's rows are exactly what vt_set_template would have written for that template at that slot, bit for bit.
 * Rows of every other slot are untouched; captured graphs stay valid (they read the cache by address).  slots: HOST array, each in
 * [0, cached frames) and none twice (else VT_ERR_ARG).  VT_ERR_STATE without a cache, or when the form batch changed since it was
 * written.  Not capturable (it stages through model scratch and copies the rows into place). */
int vt_set_template_slots(vt_model* m, const float* z_dev, const int32_t* slots, int32_t n, void* stream);

/* --- hipGraph: the whole track() device step captured once, replayed per frame -------------- */
int vt_graph_capture(vt_model* m, const float* z_dev, const float* x_dev, int32_t B,
                     const vt_outputs* out, vt_graph** g);
/* nsteps consecutive frames in ONE graph: step i is vt_forward(z_dev[i], x_dev[i], out[i]) (z_dev, or any z_dev[i], may be NULL
 * after vt_set_template; out may be NULL).  Steps run in order, so they may share buffers.  For callers that have the next
 * crops on the device already -- offline evaluation (lib/test/evaluation/running.py:56-102 reads whole sequences), or frames
 * pipelined a few deep: the runtime leaves ~7 us between two graph launches, 4 steps per graph recover ~5 % of a G128 / B=256
 * step (tools/graph_steps.py). */
int vt_graph_capture_steps(vt_model* m, int32_t nsteps, const float* const* z_dev, const float* const* x_dev, int32_t B,
                           const vt_outputs* out, vt_graph** g);
/* A graph replays kernels on its model's weights and workspaces: VT_ERR_STATE once that model has been destroyed (the graph itself can
 * still be destroyed).  Capturing from, and destroying, one model and its graphs is not thread-safe: serialise those calls. */
int vt_graph_launch(vt_graph* g, void* stream);
void vt_graph_destroy(vt_graph* g);

/* Kernel forms by group size.  Every stage has several kernel forms and picks one by the batch of the call (the
 * one-workgroup-per-frame forms once the batch fills the chip, multi-workgroup forms below); two forms of a stage agree to fp32
 * rounding (~4e-6), not bit for bit.  A caller that steps a group of N sequences as several models of N / k sequences each (one per
 * stream or per GPU: the reference shards sequences over worker processes, lib/test/evaluation/running.py:105-112) sets n = N on every
 * one of them: each shard then runs the forms the whole group would run, and a sequence's results do not depend on how the group is
 * sharded.  n = 0 (default): forms by each call's own batch.  A call with a batch larger than n uses its own batch.
 * ORDER: the value applies to LATER calls only.  Set it before vt_set_template and before any vt_graph_capture[_steps]: the template
 * cache holds the operands of the form it was written under (vt_forward(z = NULL) / vt_track_step return VT_ERR_STATE until
 * vt_set_template has run again under the new value), and captured graphs keep the forms of their capture (changing the value on a
 * model that has LIVE captured graphs returns VT_ERR_STATE; once every graph of the model has been destroyed the value is free again). */
int vt_set_form_batch(vt_model* m, int32_t n);

/* Geometry / workspace queries (host side of build_box_head: feat_sz etc.). */
int vt_query(const vt_model* m, int32_t* len_z, int32_t* len_x, int32_t* feat_sz, int32_t* channels);

/* MFMA lane-map self test: runs v_mfma_f32_16x16x4_f32 on exact integer data with an
 * asymmetric B and checks the operand / result lane maps the kernels rely on. 0 = as assumed. */
int vt_selftest_mfma(void* stream);

/* Development probe (synchronises; not part of the hot path): sustained shader clock in MHz
 * under a dense f32-MFMA loop with `waves_per_simd` waves on every SIMD, the cycles one SIMD
 * spends per v_mfma_f32_16x16x4_f32, and the wall time of the probe launch.  Used by bench.py to
 * state the clock the roofline fraction was measured at. */
int vt_probe_clock(int32_t iters, int32_t waves_per_simd, double* mhz, double* cycles_per_mfma, double* wall_us);
/* Development aid: with VT_DBG_STAMPS=1 in the environment at vt_create the transformer-block kernel
 * records s_memtime at its phase boundaries; this copies them out ([B][8][64] uint64, wave-major, synchronises). */
int vt_debug_stamps(vt_model* m, int32_t B, unsigned long long* host_out);

#ifdef __cplusplus
}
#endif
#endif /* VITTRACK_H */

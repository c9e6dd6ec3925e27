// vb_api.h -- internal interface between the C-ABI layer (vittrack.hip) and the patch-16 ViT runtime (vitb.hip: ViT-Base / -Large / -Small / -Tiny).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <string>
#include <utility>

#include "../../include/vittrack.h"

struct VbModel;

namespace vb {
using TensorMap = std::map<std::string, std::pair<const float*, int64_t>>;

// A frame slice [f0, f0 + B) of a batch of Btot frames, for graph chains that run slices concurrently (vt_graph_capture_steps,
// VT_GRAPH_CHAINS): every workspace is addressed from frame f0, tower-major buffers keep the whole batch's stride, and the
// persistent GEMMs launch at most `cus` workgroups (0 = one per CU) so that two chains share the chip.  z / x and the output
// pointers handed to stem / head are the slice's own (already offset by the caller).
struct Slice {
    size_t f0 = 0;
    int Btot = 0;
    int cus = 0;
};

// Every function returns VT_OK or a VT_ERR_* code and fills *err.
// create: channels 768, heads 12 (ViT-Base) or channels 1024, heads 16 (ViT-Large), head_channels 256, stride 16 at (template, search) =
// (128, 256) or (192, 384); the model carries its width C, its token counts and map side, every function below works on them.
int create(const vt_config* cfg, VbModel** out, std::string* err);
// create_vit (vt_create_vit): the patch-16 family by (channels, heads) = (192, 3) ViT-Tiny, (384, 6) ViT-Small (depth <= 12), or the two tuples of
// create, which it hands to create.  Anything else: VT_ERR_ARG, "unsupported ViT configuration".
int create_vit(const vt_config* cfg, VbModel** out, std::string* err);
void destroy(VbModel* m);
int load_weights(VbModel* m, const TensorMap& tm, std::string* err);
// patch_embed(z), patch_embed(x), += pos_embed, cat((z, x))  -> the model's f32 residual stream; tokens_out (optional): a copy
int stem(VbModel* m, const float* z, const float* x, int B, hipStream_t st, float* tokens_out, std::string* err, const Slice* sl = nullptr);
// The tracker's stem: template rows and search rows embedded by two GEMMs on dense operands (vb_gemm.h EPI_PATCH_ROWS), so that the template's
// operand can be cached and the search rows can come from a uint8 patch under their own (normalisation-folded) weights.
//   zsrc  Z_GIVEN: z is the fp32 template crop;  Z_CACHED: the operand rows set_template left (z unused);  Z_NONE: search rows only
//   x / xu8 (exactly one): fp32 (B,3,Tx,Tx) crop, or the uint8 (B,Tx,Tx,3) patch of vt_crop_u8* (16-byte aligned); Tx = 256 or 384
//   x_tokens_out (optional): the search rows are copied into rows [Lz, L) of this (B,L,C) matrix (L = 320: Lz = 64; L = 720: Lz = 144)
enum ZSrc { Z_GIVEN = 0, Z_CACHED = 1, Z_NONE = 2 };
int stem_rows(VbModel* m, ZSrc zsrc, const float* z, const float* x, const unsigned char* xu8, int B, hipStream_t st, float* x_tokens_out,
              std::string* err, const Slice* sl = nullptr);
// the template cache: the bf16 patch-GEMM operand rows of n templates, into slots[i] (slots == nullptr: slots 0..n-1)
int set_template(VbModel* m, const float* z, int n, const int32_t* slots, hipStream_t st, std::string* err);
// Preprocessor.process folded into the uint8 form of the patch-embedding weights (fp64; vitb.hip fold_patch_u8).  Synchronous.
int set_normalization(VbModel* m, const float* mean3, const float* std3, std::string* err);
// Candidate elimination, by key masking or compacted (vb_ce.h; include/vittrack.h vt_set_candidate_elimination / vt_ce_result).  check_ce_args: what
// can be refused without a model (n, loc, keep_ratio).  set_candidate_elimination synchronises the device and (re)allocates the stage buffers;
// ViT-Base only.  ce_result copies out what the last blocks() left for frames [0, B): removed_stage (B,LX) bytes, scores (n,B,LX) f32.
int check_ce_args(int n, const int32_t* loc, const double* keep_ratio, std::string* err);
int set_candidate_elimination(VbModel* m, int n, const int32_t* loc, const double* keep_ratio, const uint8_t* template_rows, std::string* err);
// The form the stages run in from the next blocks() on: VT_CE_MASKED (the default) or VT_CE_COMPACT (vb_ce.h); ViT-Base only.
int set_ce_form(VbModel* m, int form, std::string* err);
int ce_result(VbModel* m, int B, hipStream_t st, uint8_t* removed_stage, float* scores, std::string* err);
// Which GEMM kinds of a plain forward of B frames run the narrow 128 x 64 tile: the VT_GEMM_* bits of include/vittrack.h (vt_gemm_form)
int gemm_form(const VbModel* m, int B);
// The fp32-equivalent mode (include/vittrack.h vt_set_precision; kernels: vb_f32.h): VT_PRECISION_BF16 / VT_PRECISION_FP32.  Selecting fp32
// allocates the mode's workspaces the first time and builds the weights' piece images if the weights are loaded (else load_weights does);
// a failure leaves the model in bf16 mode.  Synchronises the device.  Refused with candidate elimination set (and the reverse).
int set_precision(VbModel* m, int precision, std::string* err);
int precision(const VbModel* m);
// blocks[0..nblocks) on the residual stream (tokens_in: optional replacement, copied in first), then the final norm:
// the search rows go to the head's input map (and to feat_out as f32 (B,Lx,C), optional); resid_out optional copy
int blocks(VbModel* m, const float* tokens_in, int B, int nblocks, hipStream_t st, float* feat_out, float* resid_out, std::string* err,
           const Slice* sl = nullptr);
// CenterPredictor towers + conv5 + sigmoid/clamp on the head's input map (feat_in: optional f32 (B,Lx,C) replacement)
int head(VbModel* m, const float* feat_in, int B, hipStream_t st, float* score, float* size, float* offset, std::string* err,
         const Slice* sl = nullptr);
}  // namespace vb

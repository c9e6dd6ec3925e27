// vt_weights.h -- vt_load_weights of the vit_48 paths: BatchNorm / LayerNorm folding in fp64 and the MFMA operand-image packers.
// Host code only.  Included by vittrack.hip after vt_model, DevBuf, fail() and HIP_TRY (it is part of that translation unit).
#pragma once

namespace {

// ------------------------------------------------------------------------------- weight packing
using TensorMap = std::map<std::string, std::pair<const float*, int64_t>>;

int need(const TensorMap& tm, const std::string& name, int64_t numel, const float** out) {
    auto it = tm.find(name);
    if (it == tm.end()) return fail(VT_ERR_MISSING_KEY, "missing key in state dict: " + name);
    if (it->second.second != numel)
        return fail(VT_ERR_MISSING_KEY, "shape mismatch for " + name + ": got " + std::to_string(it->second.second) +
                                            " elements, want " + std::to_string(numel));
    *out = it->second.first;
    return VT_OK;
}

// BN(eval) folded into the preceding conv, in double:  w' = w * g / sqrt(var + eps),
// b' = (b_conv - mean) * g / sqrt(var + eps) + beta      (Conv2d_BN.fuse, vit_dist.py:22-33)
int fold_conv_bn(const TensorMap& tm, const std::string& conv, const std::string& bn, bool conv_bias, int cout,
                 int cin, std::vector<double>& w, std::vector<double>& b) {
    const float *pw, *pb = nullptr, *g, *beta, *mu, *var;
    int rc;
    if ((rc = need(tm, conv + ".weight", (int64_t)cout * cin * 9, &pw))) return rc;
    if (conv_bias && (rc = need(tm, conv + ".bias", cout, &pb))) return rc;
    if ((rc = need(tm, bn + ".weight", cout, &g))) return rc;
    if ((rc = need(tm, bn + ".bias", cout, &beta))) return rc;
    if ((rc = need(tm, bn + ".running_mean", cout, &mu))) return rc;
    if ((rc = need(tm, bn + ".running_var", cout, &var))) return rc;
    w.resize((size_t)cout * cin * 9);
    b.resize(cout);
    for (int o = 0; o < cout; ++o) {
        const double k = (double)g[o] / std::sqrt((double)var[o] + 1e-5);
        for (int i = 0; i < cin * 9; ++i) w[(size_t)o * cin * 9 + i] = (double)pw[(size_t)o * cin * 9 + i] * k;
        b[o] = ((conv_bias ? (double)pb[o] : 0.0) - (double)mu[o]) * k + (double)beta[o];
    }
    return VT_OK;
}

// [cout][cin][3][3] -> [r][cin][s][cout]: the scalar-weight sections of vt_stem.h (stem_a)
std::vector<float> pack_conv_sections(const std::vector<double>& w, int cout, int cin) {
    std::vector<float> out((size_t)cout * cin * 9);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < cin; ++c)
            for (int s = 0; s < 3; ++s)
                for (int j = 0; j < cout; ++j)
                    out[(((size_t)r * cin + c) * 3 + s) * cout + j] = (float)w[((size_t)j * cin + c) * 9 + r * 3 + s];
    return out;
}

// [cout][cin][3][3] -> [group][tap][cin][ocg]
std::vector<float> pack_conv_groups(const std::vector<double>& w, int cout, int cin, int ocg) {
    std::vector<float> out((size_t)cout * cin * 9);
    const int ng = cout / ocg;
    for (int g = 0; g < ng; ++g)
        for (int tap = 0; tap < 9; ++tap)
            for (int c = 0; c < cin; ++c)
                for (int j = 0; j < ocg; ++j)
                    out[(((size_t)g * 9 + tap) * cin + c) * ocg + j] = (float)w[((size_t)(g * ocg + j) * cin + c) * 9 + tap];
    return out;
}

// folded conv [cout][cin][3][3] -> [oc group of 4][k][oc 4], k = tap * cin + channel, zero-padded to a multiple of 16: the A operands
// of the 4 x 4-block MFMA form (vt_head3.h SeqConvQ) -- lane l of register kg holds output channel l & 3 at k = 16 kg + (l >> 2)
void pack_conv_quads(const std::vector<double>& w, int cout, int cin, float* dst) {
    const int kp = vth::kpad16(cin);
    for (int g = 0; g < cout / 4; ++g)
        for (int k = 0; k < kp; ++k)
            for (int oc = 0; oc < 4; ++oc)
                dst[((size_t)g * kp + k) * 4 + oc] = k < 9 * cin ? (float)w[((size_t)(4 * g + oc) * cin + k % cin) * 9 + k / cin] : 0.f;
}

// folded conv [cout][cin][3][3] -> MFMA A-operand images [oc_tile][chunk][64 lanes][4] for the
// implicit GEMM of vt_head.h: element r of lane l of (ot, c) = w[oc = 16 ot + (l & 15)][ic = 4 icq + r][tap]
// with quad Q = 4 c + (l >> 4), (tap, icq) = divmod(Q, cin / 4); zero beyond cout or 9 * cin / 4 quads.
void pack_conv_image(const std::vector<double>& w, int cout, int cin, float* dst) {
    const int nq = (cin + 3) / 4, nqt = 9 * nq, nch = (nqt + 3) / 4, not_ = (cout + 15) / 16;   // cin padded to quads
    for (int ot = 0; ot < not_; ++ot)
        for (int c = 0; c < nch; ++c)
            for (int l = 0; l < 64; ++l)
                for (int r = 0; r < 4; ++r) {
                    const int oc = 16 * ot + (l & 15), Q = 4 * c + (l >> 4);
                    float v = 0.f;
                    if (oc < cout && Q < nqt) {
                        const int tap = Q / nq, ic = 4 * (Q % nq) + r;
                        if (ic < cin) v = (float)w[((size_t)oc * cin + ic) * 9 + tap];
                    }
                    dst[(((size_t)ot * nch + c) * 64 + l) * 4 + r] = v;
                }
}

// The same weights as three-piece bf16 images for vt_head3.h: [oc_tile][chunk pair][piece][64 lanes][8 bf16]; a lane's 8 values
// are its quad of chunk 2 p, then its quad of chunk 2 p + 1 (zero beyond the last chunk).  w = h + m + l exactly, by truncation
// (the split the kernels apply to activations: vth3::split3).
// x = h + m + l by truncation (vt3::split3): the bf16 bit patterns of the three pieces
void split3_host(float v, uint16_t (&pieces)[3]) {
    uint32_t xb, r1b, r2b;
    std::memcpy(&xb, &v, 4);
    float hf; const uint32_t hb = xb & 0xffff0000u; std::memcpy(&hf, &hb, 4);
    const float r1 = v - hf; std::memcpy(&r1b, &r1, 4);
    float mf; const uint32_t mb = r1b & 0xffff0000u; std::memcpy(&mf, &mb, 4);
    const float r2 = r1 - mf; std::memcpy(&r2b, &r2, 4);
    pieces[0] = (uint16_t)(xb >> 16); pieces[1] = (uint16_t)(r1b >> 16); pieces[2] = (uint16_t)(r2b >> 16);
}

// The MLP's weights as three-piece images for the block kernel's BF3 form (layout: vt_blocks.h), from the fp32 operand images
// [out tile][chunk][64 lanes][4] of the same (folded) weights.
// a K = 48 layer (fc1, qkv) from its fp32 operand image [ot][chunk 3][64 lanes][4]: [ot][ pair 0: piece x lane x 8 | chunk 2: piece x lane x 4 ]
void pack_k48_image3(const float* img1, int ntiles, uint16_t* dst) {
    constexpr int NC = vtb::NC;
    uint16_t pcs[3];
    for (int ot = 0; ot < ntiles; ++ot) {
        uint16_t* o = dst + (size_t)ot * vtb::W3_FC1_OT16 * 8;
        for (int l = 0; l < 64; ++l) {
            for (int e = 0; e < 8; ++e) {
                split3_host(img1[(((size_t)ot * NC + (e >> 2)) * 64 + l) * 4 + (e & 3)], pcs);
                for (int pc = 0; pc < 3; ++pc) o[((size_t)pc * 64 + l) * 8 + e] = pcs[pc];
            }
            for (int e = 0; e < 4; ++e) {
                split3_host(img1[(((size_t)ot * NC + 2) * 64 + l) * 4 + e], pcs);
                for (int pc = 0; pc < 3; ++pc) o[(size_t)192 * 8 + ((size_t)pc * 64 + l) * 4 + e] = pcs[pc];
            }
        }
    }
}

void pack_mlp_images3(const float* img1, const float* img2, const float* imgqkv, const float* imgproj, uint16_t* dst) {
    constexpr int NC = vtb::NC, NH = vtb::NH;
    uint16_t pcs[3];
    pack_k48_image3(imgqkv, 9, dst + (size_t)(vtb::W3_FC1_TILES + vtb::W3_FC2_TILES) * 512);
    pack_k48_image3(imgproj, NC, dst + (size_t)(vtb::W3_FC1_TILES + vtb::W3_FC2_TILES + vtb::W3_QKV_TILES) * 512);      // A3
    for (int ot = 0; ot < NH; ++ot) {           // fc1: [ot][ pair 0: piece x lane x 8 | chunk 2: piece x lane x 4 ]
        uint16_t* o = dst + (size_t)ot * vtb::W3_FC1_OT16 * 8;
        for (int l = 0; l < 64; ++l) {
            for (int e = 0; e < 8; ++e) {
                split3_host(img1[(((size_t)ot * NC + (e >> 2)) * 64 + l) * 4 + (e & 3)], pcs);
                for (int pc = 0; pc < 3; ++pc) o[((size_t)pc * 64 + l) * 8 + e] = pcs[pc];
            }
            for (int e = 0; e < 4; ++e) {
                split3_host(img1[(((size_t)ot * NC + 2) * 64 + l) * 4 + e], pcs);
                for (int pc = 0; pc < 3; ++pc) o[(size_t)192 * 8 + ((size_t)pc * 64 + l) * 4 + e] = pcs[pc];
            }
        }
    }
    uint16_t* d2 = dst + (size_t)vtb::W3_FC1_TILES * 512;
    for (int ot = 0; ot < NC; ++ot)             // fc2: [ot][pair][piece][lane][8]
        for (int p = 0; p < NH / 2; ++p)
            for (int l = 0; l < 64; ++l)
                for (int e = 0; e < 8; ++e) {
                    split3_host(img2[(((size_t)ot * NH + 2 * p + (e >> 2)) * 64 + l) * 4 + (e & 3)], pcs);
                    for (int pc = 0; pc < 3; ++pc) d2[((((size_t)ot * (NH / 2) + p) * 3 + pc) * 64 + l) * 8 + e] = pcs[pc];
                }
}

void pack_conv_image3(const std::vector<double>& w, int cout, int cin, uint16_t* dst) {
    const int nq = (cin + 3) / 4, nqt = 9 * nq, nch = (nqt + 3) / 4, ncp = (nch + 1) / 2, not_ = (cout + 15) / 16;
    for (int ot = 0; ot < not_; ++ot)
        for (int cp = 0; cp < ncp; ++cp)
            for (int l = 0; l < 64; ++l)
                for (int e = 0; e < 8; ++e) {
                    const int c = 2 * cp + (e >> 2), r = e & 3;
                    const int oc = 16 * ot + (l & 15), Q = 4 * c + (l >> 4);
                    float v = 0.f;
                    if (oc < cout && c < nch && Q < nqt) {
                        const int tap = Q / nq, ic = 4 * (Q % nq) + r;
                        if (ic < cin) v = (float)w[((size_t)oc * cin + ic) * 9 + tap];
                    }
                    uint16_t pieces[3];
                    split3_host(v, pieces);
                    for (int pc = 0; pc < 3; ++pc) dst[((((size_t)ot * ncp + cp) * 3 + pc) * 64 + l) * 8 + e] = pieces[pc];
                }
}

// nn.Linear weight (OUT, IN) -> MFMA operand images [OUT/16][IN/16][64 lanes][4]:
// element r of lane l of tile (ot, c) = W[16 ot + (l & 15)][16 c + 4 (l >> 4) + r]   (vt_common.h)
void pack_linear_image(const float* W, int OUT, int IN, float* dst) {
    const int nc = IN / 16;
    for (int ot = 0; ot < OUT / 16; ++ot)
        for (int c = 0; c < nc; ++c)
            for (int l = 0; l < 64; ++l)
                for (int r = 0; r < 4; ++r)
                    dst[(((size_t)ot * nc + c) * 64 + l) * 4 + r] = W[(size_t)(16 * ot + (l & 15)) * IN + 16 * c + 4 * (l >> 4) + r];
}

int upload(DevBuf& d, const std::vector<float>& h) {
    if (!d.p || d.n != h.size()) {
        d.release();
        int rc = d.alloc(h.size());
        if (rc) return rc;
    }
    HIP_TRY(hipMemcpy(d.p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return VT_OK;
}

// lib/test/utils/hann.py:6-16, float32 like torch
std::vector<float> hann2d(int F) {
    std::vector<float> w1(F), w((size_t)F * F);
    const float k = (float)(2.0 * M_PI / (F + 1));
    for (int i = 0; i < F; ++i) w1[i] = 0.5f * (1.0f - cosf(k * (float)(i + 1)));
    for (int y = 0; y < F; ++y)
        for (int x = 0; x < F; ++x) w[(size_t)y * F + x] = w1[y] * w1[x];
    return w;
}

// Preprocessor.process folded into layer 1 (vt_stem.h: L1In): x = u / (255 std_c) - mean_c / std_c per channel, so
// w' = w / (255 std_c), b' = b + sum_{c,tap} w (-mean_c / std_c), in fp64 from the BN-folded weights; pad value 255 mean_c.
int fold_w1u(vt_model* m, const float* mean3, const float* std3) {
    const std::vector<double>& w = m->stem_w1_f64;
    const std::vector<double>& b = m->stem_b1_f64;
    if (w.size() != 6 * 3 * 9 || b.size() != 6) return fail(VT_ERR_STATE, "layer-1 weights not loaded");
    std::vector<double> wf(w.size());
    std::vector<float> img(vts::W1U_FLOATS, 0.f);
    for (int j = 0; j < 6; ++j) {
        double bias = b[j];
        for (int c = 0; c < 3; ++c)
            for (int t = 0; t < 9; ++t) {
                const double wv = w[((size_t)j * 3 + c) * 9 + t];
                wf[((size_t)j * 3 + c) * 9 + t] = wv / (255.0 * (double)std3[c]);
                bias += wv * (-(double)mean3[c] / (double)std3[c]);
            }
        img[vts::W1U_BIAS + j] = (float)bias;
    }
    const std::vector<float> sec = pack_conv_sections(wf, 6, 3);
    std::copy(sec.begin(), sec.end(), img.begin());
    for (int c = 0; c < 3; ++c) img[vts::W1U_PAD + c] = (float)(255.0 * (double)mean3[c]);
    if (int rc = upload(m->stem_w1u, img)) return rc;
    for (int c = 0; c < 3; ++c) {       // only now: the model names the normalisation its device image holds
        m->norm_mean[c] = mean3[c];
        m->norm_std[c] = std3[c];
    }
    return VT_OK;
}

// vt_load_weights of the shape-generic path (vt_generic.h): plain row-major weights at run-time widths -- BatchNorm folded into the convs
// (Conv2d_BN.fuse, vit_dist.py:22-33) and LayerNorm-1 / -2's affine part folded into qkv / fc1, both in fp64, as on the tuned path.
int load_weights_generic(vt_model* m, const TensorMap& tm) {
    const vtg::Dims d = m->gd;
    const int C = d.C, HID = d.hid();
    int rc;
    const int sch[5] = {3, C / 8, C / 4, C / 2, C};
    for (int i = 0; i < 4; ++i) {
        const std::string p = "patch_embed.net." + std::to_string(2 * i);
        std::vector<double> w, b;
        if ((rc = fold_conv_bn(tm, p + ".c", p + ".bn", false, sch[i + 1], sch[i], w, b))) return rc;
        if ((rc = upload(m->g_stem_w[i], std::vector<float>(w.begin(), w.end())))) return rc;
        if ((rc = upload(m->g_stem_b[i], std::vector<float>(b.begin(), b.end())))) return rc;
    }
    const float* p;
    if ((rc = need(tm, "pos_embed_z", (int64_t)m->len_z * C, &p))) return rc;
    if ((rc = upload(m->pos_z, std::vector<float>(p, p + (size_t)m->len_z * C)))) return rc;
    if ((rc = need(tm, "pos_embed_x", (int64_t)m->len_x * C, &p))) return rc;
    if ((rc = upload(m->pos_x, std::vector<float>(p, p + (size_t)m->len_x * C)))) return rc;
    std::vector<float> gbp((size_t)m->cfg.depth * d.block_stride() + 2 * C);
    for (int b = 0; b < m->cfg.depth; ++b) {
        const std::string pre = "blocks." + std::to_string(b) + ".";
        float* g = gbp.data() + (size_t)b * d.block_stride();
        // y = W (gamma * n + beta) + b = (W diag gamma) n + (b + W beta)
        auto fold_ln = [&](const char* ln, const char* lin, int out, int o_w, int o_b) -> int {
            const float *G, *Be, *W, *Bi;
            int r2;
            if ((r2 = need(tm, pre + ln + ".weight", C, &G)) || (r2 = need(tm, pre + ln + ".bias", C, &Be)) ||
                (r2 = need(tm, pre + lin + ".weight", (int64_t)out * C, &W)) || (r2 = need(tm, pre + lin + ".bias", out, &Bi)))
                return r2;
            for (int o = 0; o < out; ++o) {
                double acc = (double)Bi[o];
                for (int i = 0; i < C; ++i) {
                    g[o_w + (size_t)o * C + i] = (float)((double)W[(size_t)o * C + i] * (double)G[i]);
                    acc += (double)W[(size_t)o * C + i] * (double)Be[i];
                }
                g[o_b + o] = (float)acc;
            }
            return VT_OK;
        };
        auto plain = [&](const char* lin, int out, int in, int o_w, int o_b) -> int {
            const float *W, *Bi;
            int r2;
            if ((r2 = need(tm, pre + lin + ".weight", (int64_t)out * in, &W)) || (r2 = need(tm, pre + lin + ".bias", out, &Bi))) return r2;
            std::memcpy(g + o_w, W, (size_t)out * in * sizeof(float));
            std::memcpy(g + o_b, Bi, (size_t)out * sizeof(float));
            return VT_OK;
        };
        if ((rc = fold_ln("norm1", "attn.qkv", 3 * C, d.o_wqkv(), d.o_bqkv()))) return rc;
        if ((rc = plain("attn.proj", C, C, d.o_wproj(), d.o_bproj()))) return rc;
        if ((rc = fold_ln("norm2", "mlp.fc1", HID, d.o_w1(), d.o_b1()))) return rc;
        if ((rc = plain("mlp.fc2", C, HID, d.o_w2(), d.o_b2()))) return rc;
    }
    {
        float* g = gbp.data() + (size_t)m->cfg.depth * d.block_stride();
        if ((rc = need(tm, "norm.weight", C, &p))) return rc;
        std::memcpy(g, p, C * sizeof(float));
        if ((rc = need(tm, "norm.bias", C, &p))) return rc;
        std::memcpy(g + C, p, C * sizeof(float));
    }
    if ((rc = upload(m->g_blocks, gbp))) return rc;
    std::vector<float> ghp((size_t)3 * d.tower_stride(), 0.f);
    const char* towers[3] = {"ctr", "offset", "size"};
    for (int t = 0; t < 3; ++t) {
        float* g = ghp.data() + (size_t)t * d.tower_stride();
        for (int i = 0; i < 4; ++i) {
            const std::string cn = std::string("box_head.conv") + std::to_string(i + 1) + "_" + towers[t];
            std::vector<double> w, b;
            if ((rc = fold_conv_bn(tm, cn + ".0", cn + ".1", true, d.hch(i + 1), d.hch(i), w, b))) return rc;
            for (size_t k = 0; k < w.size(); ++k) g[d.ho_w(i) + k] = (float)w[k];
            for (int o = 0; o < d.hch(i + 1); ++o) g[d.ho_b(i) + o] = (float)b[o];
        }
        const int nout = t == 0 ? 1 : 2, c4 = d.hch(4);
        const std::string c5 = std::string("box_head.conv5_") + towers[t];
        if ((rc = need(tm, c5 + ".weight", (int64_t)nout * c4, &p))) return rc;
        std::memcpy(g + d.ho_w5(), p, (size_t)nout * c4 * sizeof(float));
        if ((rc = need(tm, c5 + ".bias", nout, &p))) return rc;
        std::memcpy(g + d.ho_b5(), p, nout * sizeof(float));
    }
    if ((rc = upload(m->g_head, ghp))) return rc;
    m->weights_loaded = true;
    return VT_OK;
}

// vt_load_weights of the tuned geometries (G128 / G256 at the shipped widths): operand images for vt_stem*.h / vt_blocks.h / vt_head*.h
int load_weights_tuned(vt_model* m, const TensorMap& tm) {
    int rc;
    const int C = 48;
    // ---- stem (patch_embed.net.{0,2,4,6}.{c,bn})
    for (int i = 0; i < 4; ++i) {
        const std::string p = "patch_embed.net." + std::to_string(2 * i);
        std::vector<double> w, b;
        if ((rc = fold_conv_bn(tm, p + ".c", p + ".bn", false, STEM_CH[i + 1], STEM_CH[i], w, b))) return rc;
        if (i < 1) {   // VALU layer: [r][cin][s][cout] sections, weights become scalar operands
            if ((rc = upload(m->stem_w[i], pack_conv_sections(w, STEM_CH[i + 1], STEM_CH[i])))) return rc;
            if ((rc = upload(m->stem_b[i], std::vector<float>(b.begin(), b.end())))) return rc;
            m->stem_w1_f64 = w;
            m->stem_b1_f64 = b;
            if ((rc = fold_w1u(m, m->norm_mean, m->norm_std))) return rc;      // the uint8-patch form of layer 1
        } else {       // MFMA layers: A-operand images, bias padded to whole 16-channel tiles
            const int tiles = (STEM_CH[i + 1] + 15) / 16, nch = (9 * ((STEM_CH[i] + 3) / 4) + 3) / 4;
            std::vector<float> img((size_t)tiles * nch * 256), bias((size_t)tiles * 16, 0.f);
            pack_conv_image(w, STEM_CH[i + 1], STEM_CH[i], img.data());
            for (int o = 0; o < STEM_CH[i + 1]; ++o) bias[o] = (float)b[o];
            if ((rc = upload(m->stem_w[i], img))) return rc;
            if ((rc = upload(m->stem_b[i], bias))) return rc;
#ifdef VT_F16
            if (i >= 2 && (rc = opnd_inplace(m->stem_w[i].p, img.size()))) return rc;      // layers 3 / 4: stored operands (vt_conv.h); layer 2's image stays float4
#endif
            if (i == 1) {   // [tap][ic / 4][16 oc][ic % 4]: element = w[oc][ic][tap], zero beyond 12 x 6
                std::vector<float> k((size_t)9 * 2 * 16 * 4, 0.f);
                for (int tap = 0; tap < 9; ++tap)
                    for (int oc = 0; oc < STEM_CH[2]; ++oc)
                        for (int ic = 0; ic < STEM_CH[1]; ++ic)
                            k[(((size_t)tap * 2 + ic / 4) * 16 + oc) * 4 + ic % 4] = (float)w[((size_t)oc * STEM_CH[1] + ic) * 9 + tap];
                if ((rc = upload(m->stem_w2k, k))) return rc;
            }
            if (i == 2) {   // layer 3 as three-piece bf16 images (vt_stem_fused.h, fp32 build): [out tile 2][pair 4][piece 3][64][8 bf16]
                std::vector<uint16_t> img3((size_t)2 * 4 * 3 * 64 * 8, 0);
                pack_conv_image3(w, STEM_CH[3], STEM_CH[2], img3.data());
                std::vector<float> as_f(img3.size() / 2);
                std::memcpy(as_f.data(), img3.data(), img3.size() * 2);
                if ((rc = upload(m->stem_w3b, as_f))) return rc;
            }
            if (i == 3) {   // layer 4 as three-piece bf16 images (stem_fused with VT_STEM_BF3): [out tile 3][pair 7][piece 3][64][8 bf16]
                std::vector<uint16_t> img4((size_t)3 * 7 * 3 * 64 * 8, 0);
                pack_conv_image3(w, STEM_CH[4], STEM_CH[3], img4.data());
                std::vector<float> as_f(img4.size() / 2);
                std::memcpy(as_f.data(), img4.data(), img4.size() * 2);
                if ((rc = upload(m->stem_w4b, as_f))) return rc;
            }
        }
    }
    const float* p;
    if ((rc = need(tm, "pos_embed_z", (int64_t)m->len_z * C, &p))) return rc;
    if ((rc = upload(m->pos_z, std::vector<float>(p, p + (size_t)m->len_z * C)))) return rc;
    if ((rc = need(tm, "pos_embed_x", (int64_t)m->len_x * C, &p))) return rc;
    if ((rc = upload(m->pos_x, std::vector<float>(p, p + (size_t)m->len_x * C)))) return rc;
    // ---- transformer blocks + final norm
    std::vector<float> bp((size_t)m->cfg.depth * vtb::BLOCK_STRIDE + 2 * C);
    std::vector<uint16_t> bp3((size_t)m->cfg.depth * vtb::BLOCK3_STRIDE * 2, 0);
    for (int b = 0; b < m->cfg.depth; ++b) {
        const std::string pre = "blocks." + std::to_string(b) + ".";
        float* dst = bp.data() + (size_t)b * vtb::BLOCK_STRIDE;
        struct V { const char* name; int off; int n; };
        const V vecs[] = {{"norm1.weight", vtb::O_LN1G, C}, {"norm1.bias", vtb::O_LN1B, C},
                          {"attn.qkv.bias", vtb::O_BQKV, 3 * C}, {"attn.proj.bias", vtb::O_BPROJ, C},
                          {"norm2.weight", vtb::O_LN2G, C}, {"norm2.bias", vtb::O_LN2B, C},
                          {"mlp.fc1.bias", vtb::O_B1, 4 * C}, {"mlp.fc2.bias", vtb::O_B2, C}};
        for (const V& v : vecs) {
            if ((rc = need(tm, pre + v.name, v.n, &p))) return rc;
            std::memcpy(dst + v.off, p, v.n * sizeof(float));
        }
        // norm1 -> qkv and norm2 -> fc1: the LayerNorm's affine part is folded into the linear layer that consumes it, in
        // double (y = W (gamma * n + beta) + b = (W diag gamma) n + (b + W beta)); the kernels normalise only (vt_blocks.h).
        auto fold_ln = [&](const char* wname, int out, int o_ln_g, int o_ln_b, int o_bias, int o_w) -> int {
            const float* W;
            int rc2 = need(tm, pre + wname, (int64_t)out * C, &W);
            if (rc2) return rc2;
            std::vector<float> wf((size_t)out * C);
            for (int o = 0; o < out; ++o) {
                double acc = (double)dst[o_bias + o];
                for (int i = 0; i < C; ++i) {
                    wf[(size_t)o * C + i] = (float)((double)W[(size_t)o * C + i] * (double)dst[o_ln_g + i]);
                    acc += (double)W[(size_t)o * C + i] * (double)dst[o_ln_b + i];
                }
                dst[o_bias + o] = (float)acc;
            }
            pack_linear_image(wf.data(), out, C, dst + o_w);
            return VT_OK;
        };
        if ((rc = fold_ln("attn.qkv.weight", 3 * C, vtb::O_LN1G, vtb::O_LN1B, vtb::O_BQKV, vtb::O_WQKV))) return rc;
        if ((rc = need(tm, pre + "attn.proj.weight", C * C, &p))) return rc;
        pack_linear_image(p, C, C, dst + vtb::O_WPROJ);
        if ((rc = fold_ln("mlp.fc1.weight", 4 * C, vtb::O_LN2G, vtb::O_LN2B, vtb::O_B1, vtb::O_W1))) return rc;
        if ((rc = need(tm, pre + "mlp.fc2.weight", 4 * C * C, &p))) return rc;
        pack_linear_image(p, C, 4 * C, dst + vtb::O_W2);
        pack_mlp_images3(dst + vtb::O_W1, dst + vtb::O_W2, dst + vtb::O_WQKV, dst + vtb::O_WPROJ, bp3.data() + (size_t)b * vtb::BLOCK3_STRIDE * 2);
    }
    {
        float* dst = bp.data() + (size_t)m->cfg.depth * vtb::BLOCK_STRIDE;
        if ((rc = need(tm, "norm.weight", C, &p))) return rc;
        std::memcpy(dst, p, C * sizeof(float));
        if ((rc = need(tm, "norm.bias", C, &p))) return rc;
        std::memcpy(dst + C, p, C * sizeof(float));
    }
    if ((rc = upload(m->blocks, bp))) return rc;
#ifdef VT_F16
    {   // f16 build: the block kernels read their weight images as stored operands (vt_common.h `opnd` = h4) -- converted ONCE here,
        // on the device, by the conversion the kernels applied at every MFMA call before (bit-identical results); BLOCK_STRIDE halves
        // per block at the float layout's offsets, + 1 KiB of slack behind the last image (the staging DMA moves whole KiB)
        const size_t nflt = (size_t)m->cfg.depth * vtb::BLOCK_STRIDE;
        m->blocks3.release();
        if ((rc = m->blocks3.alloc(nflt / 2 + 256 + 256))) return rc;
        hipLaunchKernelGGL(f32_to_opnd_kernel, dim3((unsigned)((nflt / 4 + 255) / 256)), dim3(256), 0, nullptr, m->blocks.p,
                           reinterpret_cast<_Float16*>(m->blocks3.p), nflt / 4);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
    }
#else
    {
        std::vector<float> as_f(bp3.size() / 2);
        std::memcpy(as_f.data(), bp3.data(), bp3.size() * 2);
        if ((rc = upload(m->blocks3, as_f))) return rc;
    }
#endif
    // ---- head (box_head.conv{1..4}_{ctr,offset,size}.{0,1}, conv5_*)
    std::vector<float> hp((size_t)3 * vth::TOWER_STRIDE, 0.f);
#ifndef VT_F16
    std::vector<uint16_t> hp3((size_t)3 * vth3::TOWER3_STRIDE * 8, 0);
#endif
    const char* towers[3] = {"ctr", "offset", "size"};
    const int chans[5] = {48, 32, 16, 8, 4};
    const int woff[4] = {vth::O_W1, vth::O_W2, vth::O_W3, vth::O_W4};
    const int boff[4] = {vth::O_B1, vth::O_B2, vth::O_B3, vth::O_B4};
    for (int t = 0; t < 3; ++t) {
        float* dst = hp.data() + (size_t)t * vth::TOWER_STRIDE;
        for (int i = 0; i < 4; ++i) {
            const std::string cn = std::string("box_head.conv") + std::to_string(i + 1) + "_" + towers[t];
            std::vector<double> w, b;
            if ((rc = fold_conv_bn(tm, cn + ".0", cn + ".1", true, chans[i + 1], chans[i], w, b))) return rc;
            pack_conv_image(w, chans[i + 1], chans[i], dst + woff[i]);
            if (i == 2) pack_conv_quads(w, 8, 16, dst + vth::O_W3Q);
            if (i == 3) pack_conv_quads(w, 4, 8, dst + vth::O_W4Q);
#ifndef VT_F16
            {
                const int woff3[4] = {vth3::O3_W1, vth3::O3_W2, vth3::O3_W3, vth3::O3_W4};
                pack_conv_image3(w, chans[i + 1], chans[i], hp3.data() + ((size_t)t * vth3::TOWER3_STRIDE + woff3[i]) * 8);
            }
#endif
            for (int o = 0; o < chans[i + 1]; ++o) dst[boff[i] + o] = (float)b[o];
        }
        const int nout = t == 0 ? 1 : 2;
        const std::string c5 = std::string("box_head.conv5_") + towers[t];
        if ((rc = need(tm, c5 + ".weight", nout * 4, &p))) return rc;
        std::memcpy(dst + vth::O_W5, p, nout * 4 * sizeof(float));
        if ((rc = need(tm, c5 + ".bias", nout, &p))) return rc;
        std::memcpy(dst + vth::O_B5, p, nout * sizeof(float));
    }
    if ((rc = upload(m->head, hp))) return rc;
#ifdef VT_F16
    for (int t = 0; t < 3; ++t)      // the towers' conv images as stored operands, in place (biases and conv5 stay float)
        for (int i = 0; i < 4; ++i) {
            const int sizes[4] = {vth::O_B1 - vth::O_W1, vth::O_B2 - vth::O_W2, vth::O_B3 - vth::O_W3, vth::O_B4 - vth::O_W4};
            if ((rc = opnd_inplace(m->head.p + (size_t)t * vth::TOWER_STRIDE + woff[i], (size_t)sizes[i]))) return rc;
        }
#endif
#ifndef VT_F16
    {     // the three-piece bf16 images of vt_head3.h (as floats: 16-byte units x 4); F = 16 reads conv1's only
        std::vector<float> as_f(hp3.size() / 2);
        std::memcpy(as_f.data(), hp3.data(), hp3.size() * 2);
        if ((rc = upload(m->head3, as_f))) return rc;
    }
#endif
    m->weights_loaded = true;
    return VT_OK;
}

}  // namespace

"""Helper of the ViT-Base uint8-patch tests: a numpy statement of the normalisation fold of the patch embedding (vitb.hip
fold_patch_u8), with bf16 emulated by torch, and the centred relative error the token stage is held to (tests/test_gpu_vitb.py)."""
import numpy as np

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
TOL_TOKENS = 3.2e-3          # tests/test_gpu_vitb.py: the patch embedding is ONE bf16 contraction (K = 768) + an f32 add, held at twice its model


def bf16(a):
    """Round-to-nearest-even bf16 of a float array, returned as float64."""
    import torch
    return torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def operand(patches):
    """(B,S,S,3) uint8 -> (B, tokens, 768) float64 bytes in the conv weight's own k = c * 256 + r * 16 + s order."""
    B, S = patches.shape[0], patches.shape[1]
    g = S // 16
    p = patches.astype(np.float64).reshape(B, g, 16, g, 16, 3).transpose(0, 1, 3, 5, 2, 4)      # B, py, px, c, r, s
    return p.reshape(B, g * g, 768)


def fold(W, b, centre, mean=MEAN, std=STD):
    """W (N, 768) and b (N,) float32 -> (W' float64 UNROUNDED, b' float64): W' = W / (255 std_c), b' = b - sum W mean_c / std_c +
    centre * sum W', the bias from the unrounded W'."""
    W = np.asarray(W, np.float64).reshape(W.shape[0], 768)
    k255 = np.repeat(1.0 / (255.0 * np.asarray(std, np.float32).astype(np.float64)), 256)
    ms = np.repeat(np.asarray(mean, np.float32).astype(np.float64) / np.asarray(std, np.float32).astype(np.float64), 256)
    Wf = W * k255
    return Wf, np.asarray(b, np.float64) - (W * ms).sum(1) + centre * Wf.sum(1)


def tokens_truth(sd, patches, mean=MEAN, std=STD):
    """fp64 search-token rows: Preprocessor.process, patch embedding, + pos_embed_x."""
    W = np.asarray(sd["backbone.patch_embed.proj.weight"], np.float64).reshape(-1, 768)
    x = (operand(patches) / 255.0 - np.repeat(np.asarray(mean, np.float64), 256)) / np.repeat(np.asarray(std, np.float64), 256)
    return x @ W.T + np.asarray(sd["backbone.patch_embed.proj.bias"], np.float64) + np.asarray(sd["backbone.pos_embed_x"], np.float64)[0]


def tokens_folded(sd, patches, centre):
    """What the device computes on the uint8 route: bf16(byte - centre) (exact) times bf16(W'), fp32 bias b' and pos-embed added."""
    Wf, bf = fold(sd["backbone.patch_embed.proj.weight"], sd["backbone.patch_embed.proj.bias"], centre)
    acc = (operand(patches) - centre) @ bf16(Wf.astype(np.float32)).T
    return acc + bf.astype(np.float32).astype(np.float64) + np.asarray(sd["backbone.pos_embed_x"], np.float64)[0]


def tokens_fp32_route(sd, patches):
    """Today's route: the fp32 normalised crop rounded to bf16, times bf16(W)."""
    from vittracker_amd import synth
    x = synth.normalise_patches(patches)                      # (B,3,S,S) float32
    B, S = x.shape[0], x.shape[2]
    g = S // 16
    xo = x.reshape(B, 3, g, 16, g, 16).transpose(0, 2, 4, 1, 3, 5).reshape(B, g * g, 768)
    W = np.asarray(sd["backbone.patch_embed.proj.weight"], np.float32).reshape(-1, 768)
    return bf16(xo) @ bf16(W).T + np.asarray(sd["backbone.patch_embed.proj.bias"], np.float64) + np.asarray(sd["backbone.pos_embed_x"], np.float64)[0]


def rel_c(got, want):
    """Relative L2 error against the centred rows (what a LayerNorm sees)."""
    want = np.asarray(want, np.float64)
    return float(np.linalg.norm(np.asarray(got, np.float64) - want) / np.linalg.norm(want - want.mean(-1, keepdims=True)))

"""Shared by tests/test_clip_score_host.py and tests/test_clip_score_gpu.py: the shapes, the images, Pillow's levels, a numpy
int64 two-pass emulation of the integer resampler driven by the package's coefficient tables, and the tiny seeded CLIP
model with re-drawn weights."""
import numpy as np
import torch

# H x W -> R of the preprocessing cases (R = 28 with patch 14 unless a test says otherwise)
SHAPES_28 = [(64, 64), (32, 32), (8, 8), (28, 28), (17, 23), (40, 24), (24, 40), (33, 64), (100, 37), (31, 29)]
BIG_SHAPES = [(256, 256, 224), (512, 768, 224)]
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def make_images(kind, B, H, W, seed=0):
    """uint8 [B, 3, H, W]: 'noise', 'saturated' (0 / 255 only: bicubic overshoot clamps at both ends) or 'white' (255)."""
    g = np.random.default_rng(seed * 7919 + H * 131 + W)
    if kind == 'noise':
        return g.integers(0, 256, (B, 3, H, W), dtype=np.uint8)
    if kind == 'saturated':
        return (g.integers(0, 2, (B, 3, H, W)) * 255).astype(np.uint8)
    if kind == 'white':
        return np.full((B, 3, H, W), 255, np.uint8)
    raise ValueError(kind)


def pil_levels(img, R):
    """PIL.Image.resize(BICUBIC) of the shorter side to R (long side int(R * long / short)) + centre crop: uint8 [3, R, R]."""
    from PIL import Image
    _, H, W = img.shape
    short, long = (W, H) if W <= H else (H, W)
    nl = int(R * long / short)
    nh, nw = (nl, R) if W <= H else (R, nl)
    im = Image.fromarray(np.ascontiguousarray(img.transpose(1, 2, 0)), 'RGB').resize((nw, nh), Image.BICUBIC)
    a = np.asarray(im).transpose(2, 0, 1)
    top, left = (nh - R) // 2, (nw - R) // 2
    return np.ascontiguousarray(a[:, top:top + R, left:left + R])


def _pass(src, tab, axis):
    """one pass of step 5, clamp((2**21 + sum k v) >> 22, 0, 255), over ``axis`` of int64 ``src`` with table rows (lo, count, k)"""
    src = np.moveaxis(src, axis, -1)
    out = np.empty(src.shape[:-1] + (tab.shape[0],), np.int64)
    for j, row in enumerate(tab):
        lo, n = int(row[0]), int(row[1])
        acc = (src[..., lo:lo + n] * row[2:2 + n].astype(np.int64)).sum(-1) + (1 << 21)
        out[..., j] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, -1, axis)


def emulate_levels(img, R):
    """uint8 [3, R, R] from the package's tables: horizontal pass, round and clamp, vertical pass, round and clamp."""
    from diffusion_amd.metrics.clip_preprocess import tables_for
    _, H, W = img.shape
    xtab, ytab = tables_for(H, W, R)
    return _pass(_pass(img.astype(np.int64), xtab, 2), ytab, 1).astype(np.uint8)


def pixel_values(levels, mean=CLIP_MEAN, std=CLIP_STD):
    """(level / 255 - mean) / std in fp32 from uint8 [..., 3, R, R]"""
    m = np.asarray(mean, np.float32).reshape(3, 1, 1)
    s = np.asarray(std, np.float32).reshape(3, 1, 1)
    return (levels.astype(np.float32) * np.float32(1.0 / 255.0) - m) / s


def tiny_clip(seed=0, vis_hidden=128, vis_heads=2, vis_layers=2, image=28, patch=14, proj=32, text_hidden=64, text_heads=1,
              text_layers=2, eos_token_id=49407, redraw=True):
    """Seeded ``transformers.CLIPModel`` (fp32, eval).  ``redraw`` re-draws what torch's defaults leave trivial, so that no
    term can be dropped unnoticed: LayerNorm gamma ~ U(0.5, 1.5), beta and every bias ~ N(0, 0.1), class and position
    embeddings ~ N(0, 1)."""
    from transformers import CLIPConfig, CLIPModel
    torch.manual_seed(seed)
    cfg = CLIPConfig(
        text_config=dict(vocab_size=49408, hidden_size=text_hidden, intermediate_size=4 * text_hidden,
                         num_hidden_layers=text_layers, num_attention_heads=text_heads, max_position_embeddings=77,
                         hidden_act='quick_gelu', bos_token_id=49406, eos_token_id=eos_token_id, pad_token_id=1),
        vision_config=dict(hidden_size=vis_hidden, intermediate_size=4 * vis_hidden, num_hidden_layers=vis_layers,
                           num_attention_heads=vis_heads, image_size=image, patch_size=patch, hidden_act='quick_gelu'),
        projection_dim=proj)
    m = CLIPModel(cfg).float().eval()
    if redraw:
        with torch.no_grad():
            for n, p in m.named_parameters():
                if 'norm' in n and n.endswith('weight'):
                    p.uniform_(0.5, 1.5)
                elif n.endswith('bias'):
                    p.normal_(0.0, 0.1)
                elif n.endswith('class_embedding') or 'position_embedding' in n:
                    p.normal_(0.0, 1.0)
    m.requires_grad_(False)
    return m


def embeds(model, input_ids, pixel_values):
    """un-normalised (image_embeds, text_embeds) of the torch module (``CLIPModel.forward`` returns them normalised)"""
    with torch.no_grad():
        out = [model.get_image_features(pixel_values=pixel_values), model.get_text_features(input_ids=input_ids)]
    return tuple(f if torch.is_tensor(f) else f.pooler_output for f in out)   # transformers 5 wraps them in an output object


def peak_attention(model, pixel_values, target=0.2, max_doublings=12):
    """Scale the vision tower's q / k projections (weights and biases, by sqrt 2 a time) until the fp32 module's mean
    max-softmax probability over layers, heads and queries exceeds ``target``; returns that mean."""
    vm = model.vision_model
    model.set_attn_implementation('eager')   # the fused attention returns no probabilities

    def mean_peak():
        with torch.no_grad():
            out = model.vision_model(pixel_values=pixel_values, output_attentions=True)
        return float(torch.stack([a.max(-1).values.mean() for a in out.attentions]).mean())

    for _ in range(max_doublings):
        p = mean_peak()
        if p > target:
            return p
        with torch.no_grad():
            for ly in vm.encoder.layers:
                for lin in (ly.self_attn.q_proj, ly.self_attn.k_proj):
                    lin.weight.mul_(2 ** 0.5)
                    lin.bias.mul_(2 ** 0.5)
    return mean_peak()

"""The CLIP score on the HIP path: ``da_clip_preprocess`` against the integer emulation of Pillow's
resampler (tests/clip_reference.py, itself equal to PIL in tests/test_clip_score_host.py), ``da_clip_score`` against float64,
the vision / text towers against the fp32 torch module, the metric end to end against the reference route measured next to
a bf16 torch route, and the routing through ``StableDiffusion.update_metric`` / ``Trainer.eval``."""
import ctypes

import numpy as np
import pytest
import torch

import clip_reference as CR
import parity_margins

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC1   # a bf16 NaN pattern: whatever the kernel leaves unwritten stays recognisable


def _images(B, H, W):
    """B distinct images: noise, then a saturated one, then constant 255"""
    kinds = ['noise', 'saturated', 'white']
    return np.concatenate([CR.make_images(kinds[b % 3], 1, H, W, seed=b) for b in range(B)])


PRE_CASES = [(H, W, R, P, B) for (H, W) in CR.SHAPES_28 for (R, P) in ((28, 14), (32, 16)) for B in (1, 3)] \
    + [(256, 256, 224, 14, 2), (512, 768, 224, 14, 1)]


@pytest.mark.parametrize('H,W,R,P,B', PRE_CASES)
def test_preprocess_levels_layout_and_guards(dev, H, W, R, P, B):
    from diffusion_amd import ops
    img = _images(B, H, W)
    ref = np.stack([CR.pixel_values(CR.emulate_levels(i, R)) for i in img])   # fp32 [B, 3, R, R] from the exact levels
    d_img = torch.from_numpy(img).to(dev)
    # kind 1: three fp32 operations on an exact level; one wrong level would be 1 / (255 * 0.28) = 1.4e-2
    pv = torch.full((B, 3, R, R), float('nan'), device=dev)
    ops.clip_preprocess(d_img, R, P, pv, 1, CR.CLIP_MEAN, CR.CLIP_STD)
    err = np.abs(pv.cpu().numpy().astype(np.float64) - ref)
    bound = 2.0 ** -20 + 2.0 ** -22 * np.abs(ref)
    print(f'kind 1 max err {err.max():.3e} (bound at that value {bound.flat[err.argmax()]:.3e})')
    assert (err <= bound).all(), float(err.max())
    # kind 0: bf16 round-to-nearest-even of those values in the patch-matrix layout, zeros in class rows and pad columns,
    # nothing outside the matrix touched
    G = R // P
    Np, Kp, guard = G * G, ops.clip_patch_cols(P), 3
    rows = B * (Np + 1)
    buf = torch.full((rows + 2 * guard, Kp), NAN_BITS, dtype=torch.int16, device=dev)
    out = buf[guard:guard + rows].view(torch.bfloat16)
    ops.clip_preprocess(d_img, R, P, out, 0, CR.CLIP_MEAN, CR.CLIP_STD)
    got = buf.cpu()
    assert (got[:guard] == NAN_BITS).all() and (got[guard + rows:] == NAN_BITS).all()
    mat = got[guard:guard + rows].view(B, Np + 1, Kp)
    assert (mat[:, 0] == 0).all(), 'class-token rows must be exact zeros'
    assert (mat[:, :, 3 * P * P:] == 0).all(), 'pad columns must be exact zeros'
    want = pv.cpu().view(B, 3, G, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(B, Np, 3 * P * P).to(torch.bfloat16)
    assert torch.equal(mat[:, 1:, :3 * P * P], want.view(torch.int16))


def test_preprocess_rejections(dev):
    from diffusion_amd import _lib, ops
    lib = _lib.load()
    img = torch.zeros(1, 3, 64, 64, dtype=torch.uint8, device=dev)
    tab = torch.zeros(448, 8, dtype=torch.int32, device=dev)
    out = torch.zeros(1 << 20, dtype=torch.float32, device=dev)
    f3 = ctypes.c_float * 3
    mean, std = f3(*CR.CLIP_MEAN), f3(*CR.CLIP_STD)

    def rc(H=64, W=64, R=28, P=14, kind=0, off=0):
        return lib.da_clip_preprocess(img.data_ptr(), 1, H, W, R, P, tab.data_ptr(), 8, tab.data_ptr(), 8, mean, std,
                                      out.data_ptr() + off, kind, torch.cuda.current_stream().cuda_stream)

    assert rc(R=30) == 1                      # R % P != 0
    assert rc(R=66, P=33) == 1                # P > 32
    assert rc(R=462) == 1                     # R > 448
    assert rc(H=0) == 1 and rc(W=0) == 1      # sides < 1
    assert rc(H=65536) == 1 and rc(W=65536) == 1
    assert rc(off=8) == 1 and rc(off=2) == 1  # kind 0 needs 16 bytes
    assert rc(kind=1, off=2) == 1             # kind 1 needs 4 bytes
    assert rc(kind=2) == 1
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0      # nothing was launched
    with pytest.raises(ValueError):
        ops.clip_preprocess(img, 30, 14, out[:10].view(torch.bfloat16).view(-1, 4), 0, CR.CLIP_MEAN, CR.CLIP_STD)


@pytest.mark.parametrize('D', [8, 33, 768])
@pytest.mark.parametrize('B', [1, 5, 67])
def test_score_against_float64(dev, B, D):
    from diffusion_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + D)
    a = torch.randn(B, D + 5, generator=g)
    b = torch.randn(B, D + 3, generator=g)
    b[1::2, :D] = -a[1::2, :D] + 0.3 * b[1::2, :D]   # pairs with a negative cosine: nothing is clamped per sample
    a64, b64 = a[:, :D].double(), b[:, :D].double()
    ref = 100.0 * (a64 * b64).sum(-1) / (a64.norm(dim=-1) * b64.norm(dim=-1))
    da, db = a.to(dev)[:, :D], b.to(dev)[:, :D]    # strided leading dimensions
    scores = torch.full((B,), float('nan'), device=dev)
    state = torch.zeros(2, device=dev)
    ops.clip_score(da, db, scores, state)
    s1, st1 = scores.cpu(), state.cpu()
    err = (s1.double() - ref).abs().max().item()
    bound = 100.0 * (2 * D + 16) * 2.0 ** -24       # sequential-summation bound: one dot product and two norms
    print(f'B {B} D {D}: max err {err:.3e} bound {bound:.3e}')
    assert err <= bound
    if B > 1:
        assert ref.min() < 0 and s1.min() < 0
    seq = np.float32(0.0)
    for x in s1.numpy():
        seq = np.float32(seq + x)                   # state[0]: the scores added in index order
    assert st1[0].item() == float(seq) and st1[1].item() == float(B)
    scores2 = torch.empty_like(scores)
    ops.clip_score(da, db, scores2, state)          # accumulates; a repeated call is bit-identical
    assert torch.equal(scores2.cpu().view(torch.int32), s1.view(torch.int32))
    st2 = state.cpu()
    assert st2[0].item() == float(np.float32(np.float32(st1[0].item()) + seq)) and st2[1].item() == float(2 * B)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@pytest.mark.parametrize('hidden,heads,image,src', [(128, 2, 28, 64), (1024, 16, 224, 256)])
def test_towers_match_the_fp32_module(dev, hidden, heads, image, src):
    """image_embeds / text_embeds against the fp32 torch module on the same pixel_values / ids: rel-L2 < 2e-2, the bound of
    tests/test_text_hip_gpu.py for this kernel set at this depth.  224 / 14 gives 257 tokens: a query tile with a tail of 1."""
    from diffusion_amd.models.clip_vision_hip import CLIPTextEmbedHIP, CLIPVisionHIP
    B = 2
    model = CR.tiny_clip(seed=hidden, vis_hidden=hidden, vis_heads=heads, image=image).to(dev)
    img = _images(B, src, src)
    pv = torch.from_numpy(np.stack([CR.pixel_values(CR.emulate_levels(i, image)) for i in img])).to(dev)
    peak = CR.peak_attention(model, pv)
    print(f'mean max-softmax probability {peak:.3f}')
    assert peak > 0.2
    ids = torch.randint(0, 49000, (B, 77), generator=torch.Generator().manual_seed(1))
    ids[0, 20:] = 49407
    ids[1, 76] = 49407
    ids = ids.to(dev)
    ref_img, ref_txt = CR.embeds(model, ids, pv)
    got_img = CLIPVisionHIP(model, dev)(torch.from_numpy(img).to(dev), CR.CLIP_MEAN, CR.CLIP_STD)
    got_txt = CLIPTextEmbedHIP(model, dev)(ids)
    assert got_img.shape == ref_img.shape and got_img.dtype == torch.float32
    assert got_txt.shape == ref_txt.shape and got_txt.dtype == torch.float32
    ri, rt = _rel(got_img, ref_img), _rel(got_txt, ref_txt)
    parity_margins.record(f'clip_towers_h{hidden}', tolerances={'rel_l2': 2e-2}, image_embeds=ri, text_embeds=rt, peak=peak)
    print(f'rel-L2 image {ri:.3e} text {rt:.3e}')
    assert ri < 2e-2 and rt < 2e-2, (ri, rt)


def test_unsupported_head_dim_is_an_error_not_a_fallback(dev):
    from diffusion_amd.models.clip_vision_hip import CLIPVisionHIP
    with pytest.raises(ValueError):
        CLIPVisionHIP(CR.tiny_clip(vis_hidden=128, vis_heads=4, redraw=False), dev)


def _score64(img, txt):
    img, txt = img.double(), txt.double()
    return 100.0 * (img / img.norm(dim=-1, keepdim=True) * (txt / txt.norm(dim=-1, keepdim=True))).sum(-1)


def test_metric_end_to_end_against_the_reference_route(dev):
    """Two updates (B = 3 with strings, B = 2 with ids) per seed, 4 seeds = 20 pairs.  Reference: the installed
    CLIPImageProcessor, the fp32 module, torchmetrics' formula in float64.  Yardstick: the same module with bf16 weights and
    activations on the same inputs; the HIP route's worst per-pair deviation from fp32 must be <= 3 x the bf16 route's (the
    HIP path also rounds to bf16 between kernels, where torch keeps fp32 inside its fused ops).
    Measured on an MI355X: HIP 0.306, bf16 torch 0.389 (profiles/clip_score_margins.json)."""
    import copy
    from transformers import CLIPImageProcessor
    from diffusion_amd.metrics.clip_score import CLIPScore
    from diffusion_amd.models.text import ByteTokenizer
    tok, proc = ByteTokenizer(), CLIPImageProcessor(size={'shortest_edge': 28}, crop_size={'height': 28, 'width': 28})
    captions = ['a photo of a cat', 'two dogs on a beach at dusk', 'x', 'the quick brown fox jumps over the lazy dog',
                'an oil painting of a lighthouse']
    dev_hip = dev_bf16 = 0.0
    for seed in range(4):
        model = CR.tiny_clip(seed=seed).to(dev)
        metric = CLIPScore(model=model, tokenizer=tok, device=dev)
        imgs = torch.from_numpy(CR.make_images('noise', 5, 64, 64, seed=seed))
        ids = tok(captions, padding='max_length', max_length=77, truncation=True, return_tensors='pt')['input_ids']
        s_a = metric.update(imgs[:3], captions[:3])
        s_b = metric.update([i for i in imgs[3:]], ids[3:])
        got = torch.cat([s_a, s_b]).cpu().double()
        pv = proc(images=[i for i in imgs], return_tensors='pt')['pixel_values'].to(dev)
        with torch.no_grad():
            o = model(input_ids=ids.to(dev), pixel_values=pv)
            ref = _score64(o.image_embeds, o.text_embeds).cpu()
            m16 = copy.deepcopy(model).to(torch.bfloat16)
            o16 = m16(input_ids=ids.to(dev), pixel_values=pv.to(torch.bfloat16))
            s16 = _score64(o16.image_embeds, o16.text_embeds).cpu()
        dev_hip = max(dev_hip, (got - ref).abs().max().item())
        dev_bf16 = max(dev_bf16, (s16 - ref).abs().max().item())
        # the state is the pooled mean of the scores (5 fp32 additions of values below 100: 5 * 100 * 2**-24 = 3e-5)
        assert abs(float(metric.compute()) - max(got.mean().item(), 0.0)) <= 1e-4
        assert metric.state[1].item() == 5.0
    parity_margins.record('clip_score_e2e', tolerances={'hip_over_bf16_torch': 3.0}, hip_worst=dev_hip, bf16_torch_worst=dev_bf16)
    print(f'worst per-pair deviation from fp32: HIP {dev_hip:.4e}, bf16 torch {dev_bf16:.4e}')
    assert dev_hip <= 3.0 * dev_bf16, (dev_hip, dev_bf16)


def test_update_argument_checks(dev):
    from diffusion_amd.metrics.clip_score import CLIPScore
    metric = CLIPScore(model=CR.tiny_clip(redraw=False), device=dev)
    a, b = torch.zeros(3, 64, 64, dtype=torch.uint8), torch.zeros(3, 32, 64, dtype=torch.uint8)
    with pytest.raises(ValueError):
        metric.update([a, b], ['x', 'y'])          # mixed sizes
    with pytest.raises(ValueError):
        metric.update(a[None].float(), ['x'])      # not uint8
    with pytest.raises(ValueError):
        metric.update(a[None], ['x', 'y'])         # counts differ
    assert metric.state.tolist() == [0.0, 0.0]


def test_trainer_eval_routes_generated_images_to_the_metric(dev):
    """``Trainer.eval`` -> ``eval_forward`` (one batch of generated images per guidance scale) -> ``update_metric`` -> the metric,
    against feeding ``outputs[3][scale]`` to a fresh metric by hand; the MeanSquaredError entries are what they are without it."""
    from diffusion_amd.metrics.clip_score import CLIPScore
    from diffusion_amd.models.composer_shim import MeanSquaredError
    from diffusion_amd.models.models import stable_diffusion_2
    from diffusion_amd.optim import FusedAdamW
    from diffusion_amd.trainer import Trainer
    clip = CR.tiny_clip(seed=5).to(dev)
    model = stable_diffusion_2(model_name='tiny', pretrained=False, fsdp=False, encode_latents_in_fp16=False,
                               val_metrics=[MeanSquaredError(), CLIPScore(model=clip, device=dev)],
                               val_guidance_scales=[1.0, 3.0])
    keys = ['CLIPScore-scale-1p0', 'CLIPScore-scale-3p0']
    assert all(k in model.val_metrics for k in keys)
    assert model.val_metrics[keys[0]]._shared is model.val_metrics[keys[1]]._shared
    tok = model.tokenizer
    g = torch.Generator().manual_seed(4)
    texts = [['a red cube', 'a blue ball'], ['green', 'a yellow house by the sea']]
    evalset = [{'image': torch.randn(2, 3, 64, 64, generator=g),
                'captions': tok(t, padding='max_length', max_length=77, truncation=True, return_tensors='pt')['input_ids']}
               for t in texts]
    opt = FusedAdamW(lr=1e-3, weight_decay=0.01, unet=model.unet)
    tr = Trainer(model, train_dataloader=None, optimizers=opt, max_duration='1ba', eval_dataloader=evalset, log_every=1000)
    seen = []
    inner = model.eval_forward

    def recording(batch, outputs=None):
        out = inner(batch, outputs)
        seen.append((batch, out))
        return out

    model.eval_forward = recording
    torch.manual_seed(11)
    out = tr.eval()
    assert len(seen) == 2
    for scale, key in zip((1.0, 3.0), keys):
        val = out['metrics/eval/' + key]
        assert np.isfinite(val)
        fresh = CLIPScore(model=clip, device=dev)
        for batch, o in seen:
            caps = [tok.decode(c, skip_special_tokens=True) for c in batch['captions']]
            fresh.update((o[3][scale] * 255).to(torch.uint8), caps)
        assert val == pytest.approx(float(fresh.compute()), rel=1e-6, abs=1e-5), (val, float(fresh.compute()))
    assert [tok.decode(c) for c in evalset[1]['captions']] == texts[1]
    # the same evaluation without the CLIP metric: every MeanSquaredError entry unchanged
    mse = {k: v for k, v in out.items() if 'MeanSquaredError' in k}
    assert 'metrics/eval/MeanSquaredError' in mse and len(mse) >= 2
    for k in keys:
        del model.val_metrics[k]
    torch.manual_seed(11)
    again = tr.eval()
    assert sorted(again) == sorted(mse)
    for k, v in mse.items():
        assert again[k] == pytest.approx(v, rel=1e-5), k

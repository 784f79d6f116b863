"""CPU side of the CLIP score: the package's integer coefficient tables reproduce Pillow's 8-bit
bicubic resize bit for bit, the pixel values are the installed CLIPImageProcessor's, the pooled text row is transformers',
and the metric object's protocol (hydra aliases, deepcopy, compute, no CPU path)."""
import copy

import numpy as np
import pytest
import torch

import clip_reference as CR

CASES = [(h, w, 28) for h, w in CR.SHAPES_28] + CR.BIG_SHAPES


@pytest.mark.parametrize('H,W,R', CASES)
def test_tables_reproduce_pil_exactly(H, W, R):
    """Tables from the product, the two integer passes restated in clip_reference._pass: equal to PIL.Image.resize(BICUBIC) +
    centre crop on noise, on saturated 0 / 255 images (overshoot clamps at both ends) and on constant 255."""
    for kind in ('noise', 'saturated', 'white'):
        img = CR.make_images(kind, 1, H, W)[0]
        got, ref = CR.emulate_levels(img, R), CR.pil_levels(img, R)
        assert got.shape == ref.shape == (3, R, R)
        assert np.array_equal(got, ref), (kind, int((got != ref).sum()))
        if kind == 'white':
            assert (got == 255).all()


def test_identity_table_and_geometry():
    from diffusion_amd.metrics.clip_preprocess import bicubic_table, resize_geometry
    t = bicubic_table(28, 28, 28)
    assert t.shape == (28, 3) and all(tuple(r) == (j, 1, 1 << 22) for j, r in enumerate(t))
    assert resize_geometry(512, 768, 224) == (224, 336, 0, 56)
    assert resize_geometry(100, 37, 28) == (75, 28, 23, 0)
    t = bicubic_table(100, 75, 28)   # rows of the 28 cropped indices only, windows inside the source
    assert t.shape[0] == 28 and (t[:, 0] >= 0).all() and (t[:, 0] + t[:, 1] <= 100).all()
    assert (t[:, 2:].sum(1) - (1 << 22)).__abs__().max() <= t.shape[1]   # the rounded weights sum to 1 within a unit each


def test_pixel_values_match_the_image_processor():
    from transformers import CLIPImageProcessor
    img = CR.make_images('noise', 2, 100, 37)
    ref = CLIPImageProcessor()(images=[torch.from_numpy(i) for i in img], return_tensors='pt')['pixel_values'].numpy()
    got = np.stack([CR.pixel_values(CR.emulate_levels(i, 224)) for i in img])
    assert ref.shape == got.shape == (2, 3, 224, 224)
    assert np.abs(ref - got).max() <= 1e-6, np.abs(ref - got).max()


@pytest.mark.parametrize('eos_token_id', [2, 7])
def test_eos_index_is_the_row_clip_text_model_pools(eos_token_id):
    from transformers import CLIPTextConfig, CLIPTextModel
    from diffusion_amd.models.clip_vision_hip import eos_index
    torch.manual_seed(eos_token_id)
    cfg = CLIPTextConfig(vocab_size=64, hidden_size=32, intermediate_size=64, num_hidden_layers=1, num_attention_heads=1,
                         max_position_embeddings=16, bos_token_id=0, eos_token_id=eos_token_id, pad_token_id=1)
    te = CLIPTextModel(cfg).eval()
    ids = torch.randint(8, 40, (5, 16))
    for b, pos in enumerate([3, 15, 1, 9, 9]):   # an end token per row (the legacy rule pools the largest id), repeated after it
        ids[b, pos:] = 63 if eos_token_id == 2 else eos_token_id
    ids[3, 2] = 50   # a larger id before the end token: only the legacy argmax rule must ignore where eos_token_id sits
    with torch.no_grad():
        out = te(input_ids=ids)
    idx = eos_index(ids, eos_token_id)
    assert idx.tolist() == [3, 15, 1, 9, 9]
    assert torch.equal(out.last_hidden_state[torch.arange(5), idx], out.pooler_output)


@pytest.fixture(scope='module')
def tiny():
    return CR.tiny_clip()


def test_hydra_aliases_resolve():
    from diffusion_amd import hydra_lite
    from diffusion_amd.metrics.clip_score import CLIPScore
    assert hydra_lite.resolve_target('torchmetrics.multimodal.clip_score.CLIPScore') is CLIPScore
    assert hydra_lite.resolve_target('torchmetrics.multimodal.CLIPScore') is CLIPScore
    assert CLIPScore.__name__ == 'CLIPScore'


def test_deepcopy_shares_towers_and_separates_state(tiny):
    from diffusion_amd.metrics.clip_score import CLIPScore
    m = CLIPScore(model=tiny, device='cpu')
    m.state.copy_(torch.tensor([3.0, 1.0]))
    c = copy.deepcopy(m)
    c.guidance_scale = 3.0
    assert c._shared is m._shared and c._shared['model'] is tiny
    w, cw = tiny.visual_projection.weight, c._shared['model'].visual_projection.weight
    assert w.data_ptr() == cw.data_ptr()
    assert c.state.data_ptr() != m.state.data_ptr() and torch.equal(c.state, m.state)
    c.reset()
    assert m.state.tolist() == [3.0, 1.0] and c.state.tolist() == [0.0, 0.0]
    assert not hasattr(m, 'guidance_scale')
    assert list(m.parameters()) == []   # the towers never reach an optimizer through the model that owns the metric


def test_no_cpu_path(tiny):
    from diffusion_amd.metrics.clip_score import CLIPScore
    from diffusion_amd.models.clip_vision_hip import CLIPVisionHIP
    m = CLIPScore(model=tiny, device='cpu')
    with pytest.raises(RuntimeError):
        m.update(torch.zeros(1, 3, 8, 8, dtype=torch.uint8), ['a'])
    with pytest.raises(RuntimeError):
        CLIPVisionHIP(tiny, device='cpu')


def test_compute_on_hand_set_state(tiny):
    from diffusion_amd.metrics.clip_score import CLIPScore
    m = CLIPScore(model=tiny, device='cpu')
    m.state.copy_(torch.tensor([-7.5, 3.0]))   # a negative mean is clamped (torchmetrics clamps in compute, not per sample)
    assert float(m.compute()) == 0.0
    m.reset()
    for s, n in ((30.0, 3.0), (-4.0, 2.0)):    # two updates -> the pooled mean, not the mean of the means
        m.state += torch.tensor([s, n])
    assert float(m.compute()) == pytest.approx(26.0 / 5.0)
    m.reset()
    assert m.state.tolist() == [0.0, 0.0]


def test_unknown_name_gives_a_warning_not_a_download(monkeypatch):
    from diffusion_amd.metrics import clip_score as CS
    monkeypatch.setattr(CS, '_random_init', lambda: (CR.tiny_clip(redraw=False), object()))
    with pytest.warns(UserWarning, match='RANDOM-INIT'):
        m = CS.CLIPScore(device='cpu')
    assert m.mean == CR.CLIP_MEAN and m.std == CR.CLIP_STD

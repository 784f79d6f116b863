"""The COCO evaluation route end to end on the GPU: a COCO-style MDS directory -> ``build_streaming_cocoval_dataloader`` ->
``StableDiffusion.ingest_raw`` (``ops.image_resize``) against the float64 restatement of tests/resize_reference.py on the
decoded pixels, then ``Trainer.eval()`` on that loader with a CLIP score and ``LogDiffusionImages``."""
import io

import numpy as np
import pytest
import torch

import clip_reference as CR
import resize_reference as RR

pytestmark = pytest.mark.gpu

SIZES = [(48, 80), (97, 64), (33, 70), (64, 64), (120, 51)]   # (h, w) of the five images
R = 64


def _encoded(pil, fmt):
    buf = io.BytesIO()
    pil.save(buf, format=fmt)
    return buf.getvalue()


@pytest.fixture(scope='module')
def coco(tmp_path_factory):
    """five images of different sizes and modes - a JPEG, a greyscale JPEG, a palette PNG, one ``pil``-encoded, an RGBA PNG -
    each with two captions.  A writer gives all its shards one encoding per column, so each encoding is written as a
    directory of its own and the shards are then gathered under one index (a reader follows every shard's own column table).
    Returns the directory, the RGB pixels a worker must decode, and the captions."""
    pytest.importorskip('PIL.Image')
    import json
    import shutil
    from PIL import Image
    from diffusion_amd.datasets.image_ingest import decode_rgb
    from diffusion_amd.datasets.mds import write_mds
    d = tmp_path_factory.mktemp('coco_val')
    src = [RR.seeded_image(h, w, 500 + i) for i, (h, w) in enumerate(SIZES)]
    rgba = Image.fromarray(src[4]).convert('RGBA')
    values = [_encoded(Image.fromarray(src[0]), 'JPEG'), _encoded(Image.fromarray(src[1][..., 0]), 'JPEG'),
              _encoded(Image.fromarray(src[2]).convert('P'), 'PNG'), Image.fromarray(src[3]), _encoded(rgba, 'PNG')]
    captions = [[f'a photo of thing {i}', f'another view of thing {i}'] for i in range(5)]
    shards = []
    for k, (enc, idx) in enumerate((('jpeg', [0, 1]), ('png', [2]), ('pil', [3]), ('png', [4]))):
        part = d / f'part{k}'
        write_mds(str(part), {'image': enc, 'captions': 'json'}, [{'image': values[i], 'captions': captions[i]} for i in idx])
        with open(part / 'index.json') as f:
            info = json.load(f)['shards'][0]
        name = f'shard.{k:05d}.mds'
        shutil.copy(part / info['raw_data']['basename'], d / name)
        shutil.rmtree(part)
        info['raw_data']['basename'] = name
        shards.append(info)
    with open(d / 'index.json', 'w') as f:
        json.dump({'version': 2, 'shards': shards}, f)
    pixels = [src[3] if i == 3 else decode_rgb(values[i]) for i in range(5)]
    assert [p.shape for p in pixels] == [(h, w, 3) for h, w in SIZES]
    assert np.array_equal(pixels[1][..., 0], pixels[1][..., 2])   # the greyscale one, converted
    return str(d), pixels, captions


@pytest.fixture(scope='module')
def model(dev):
    from diffusion_amd.metrics.clip_score import CLIPScore
    from diffusion_amd.models.composer_shim import MeanSquaredError
    from diffusion_amd.models.models import stable_diffusion_2
    clip = CR.tiny_clip(seed=5).to(dev)
    return stable_diffusion_2(model_name='tiny', pretrained=False, fsdp=False, encode_latents_in_fp16=False,
                              val_metrics=[MeanSquaredError(), CLIPScore(model=clip, device=dev)], val_guidance_scales=[3.0])


def _loader(coco, **kw):
    from diffusion_amd.datasets import build_streaming_cocoval_dataloader
    return build_streaming_cocoval_dataloader(batch_size=2, remote=None, local=coco[0], resize_size=R, num_workers=0, **kw)


@pytest.mark.parametrize('use_crop', [False, True])
def test_loader_batches_through_ingest_raw(coco, model, dev, use_crop):
    """``batch['image']`` is the reference's tensor: fp32 [B, 3, 64, 64] on the device, in [0, 1], within 1e-5 (the kernel's
    bound against float64) of the restated transform of the decoded pixels; captions are the first caption's ids"""
    _, pixels, captions = coco
    sw = (0, 0, 1) if use_crop else (1, 1, 1)
    batches = list(_loader(coco, use_crop=use_crop))
    assert [b['image_off'].numel() for b in batches] == [2, 2, 1]   # three batches, the last of one image
    i = 0
    for batch in batches:
        fed = model.ingest_raw(batch)
        assert not {'image_raw', 'image_off', 'image_hw', 'image_size', 'image_transform', 'image_nhwc8'} & set(fed)
        image = fed['image']
        B = image.shape[0]
        assert image.dtype == torch.float32 and image.is_cuda and tuple(image.shape) == (B, 3, R, R)
        got = image.cpu().numpy()
        assert got.min() >= 0.0 and got.max() <= 1.0
        for b in range(B):
            d = float(np.abs(got[b].astype(np.float64) - RR.resize_f64(pixels[i], R, R, *sw)).max())
            print(f'use_crop={use_crop} image {i} {pixels[i].shape[:2]}: {d:.3e}')
            assert d <= 1e-5, (i, d)
            want = model.tokenizer(captions[i][0], padding='max_length', max_length=77, truncation=True)['input_ids']
            assert fed['captions'][b].tolist() == list(want)
            i += 1
    assert i == 5


def test_trainer_eval_on_the_loader_scores_generated_images_and_logs_prompt_images(coco, model, dev, tmp_path):
    from PIL import Image
    from diffusion_amd.callbacks import LogDiffusionImages
    from diffusion_amd.optim import FusedAdamW
    from diffusion_amd.trainer import Trainer
    key = 'CLIPScore-scale-3p0'
    assert key in model.val_metrics
    cb = LogDiffusionImages(prompts=['a', 'b'], size=64, num_inference_steps=2)
    opt = FusedAdamW(lr=1e-3, weight_decay=0.01, unet=model.unet)
    tr = Trainer(model, train_dataloader=None, optimizers=opt, max_duration='1ba', eval_dataloader=_loader(coco),
                 callbacks=[cb], save_folder=str(tmp_path), log_every=1000)
    received, generations = [], []
    metric = model.val_metrics[key]
    inner_update, inner_generate = metric.update, model.generate

    def update(images, text):
        received.append((tuple(images.shape), images.dtype, list(text)))
        return inner_update(images, text)

    def generate(*a, **kw):
        generations.append(kw)
        return inner_generate(*a, **kw)

    metric.update, model.generate = update, generate
    try:
        torch.manual_seed(11)
        out = tr.eval()
    finally:
        del metric.update, model.generate
    assert np.isfinite(out['metrics/eval/MeanSquaredError']) and np.isfinite(out['metrics/eval/' + key])
    # the metric received five generated 64 x 64 images, with the first captions as text
    assert [s for s, _, _ in received] == [(2, 3, R, R), (2, 3, R, R), (1, 3, R, R)]
    assert all(dt == torch.uint8 for _, dt, _ in received)
    assert [t for _, _, text in received for t in text] == [c[0] for c in coco[2]]
    assert metric.state[1].item() == 5.0
    # the callback generated once, for its two prompts, and wrote two 64 x 64 PNGs
    mine = [kw for kw in generations if kw.get('num_inference_steps') == 2]
    assert len(mine) == 1 and len(generations) == 4
    assert mine[0]['height'] == 64 and mine[0]['width'] == 64 and mine[0]['seed'] == 1138 and mine[0]['progress_bar'] is False
    assert tuple(mine[0]['tokenized_prompts'].shape) == (2, 77)
    folder = tmp_path / 'images' / 'ba0'
    assert sorted(p.name for p in folder.iterdir()) == ['0.png', '1.png']
    for k in (0, 1):
        with Image.open(folder / f'{k}.png') as im:
            assert im.size == (64, 64) and im.mode == 'RGB'
    logged = [d for d in tr.logs if any(str(k).startswith('images/') for k in d)]
    assert len(logged) == 1
    assert logged[0]['images/a'] == str(folder / '0.png') and logged[0]['images/b'] == str(folder / '1.png')

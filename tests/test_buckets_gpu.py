"""GPU tests of aspect-ratio bucketed training end to end: the bucketed dataloader into ``ingest_raw``, a
training step per bucket shape against the same step through the single-shape rectangular path, a ``Trainer`` run that
alternates shapes (repeatable, resumable with the crop / flip draws on, and the same under graph replay), and the bucketed
latent columns of tools/precompute_latents.py.

The tiny U-Net and VAE, the 5-entry table ``bucket_table(128, 64, 64, 256)`` and the 40-image directory of
tests/bucket_data.py (four aspect ratios, 8 to 12 images per bucket), batch 4.  The project's reductions are fixed-order, so
every comparison here is bit for bit."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from bucket_data import BUCKET_KW, T5, write_image_mds

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, 'yamls', 'hydra-yamls', 'SD-2-base-512-buckets.yaml')


@pytest.fixture(scope='module')
def image_dir(tmp_path_factory):
    pytest.importorskip('PIL.Image')
    return write_image_mds(str(tmp_path_factory.mktemp('buckets') / 'raw'))


@pytest.fixture(scope='module')
def model(dev):
    from diffusion_amd.models.models import stable_diffusion_2
    torch.manual_seed(11)
    m = stable_diffusion_2(model_name='tiny', pretrained=False, precomputed_latents=False, fsdp=False)
    assert m.vae_hip is not None
    return m


def _loader(image_dir, **kw):
    from diffusion_amd.datasets.laion.laion import build_streaming_laion_dataloader
    args = dict(local=image_dir, batch_size=4, resize_size=128, aspect_buckets=BUCKET_KW, seed=11)
    args.update(kw)
    return build_streaming_laion_dataloader(**args)


def _bits(x):
    return x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize('augment', [False, True], ids=['centre', 'crop_flip'])
def test_every_batch_of_an_epoch_is_ingested_at_its_bucket(image_dir, model, dev, augment):
    """``model.ingest_raw`` on each batch of one epoch against the op by hand on the same packed samples: the rectangular
    entry at the batch's bucket, or the augmenting entry with the batch's ``image_aug``"""
    from diffusion_amd import ops
    dl = _loader(image_dir, **(dict(random_crop=True, flip_prob=0.5) if augment else {}))
    seen = set()
    for b in dl:
        Rh, Rw = b['image_size']
        assert (Rh, Rw) in T5 and ('image_aug' in b) == augment
        off, hw = b['image_off'], b['image_hw']
        hand = torch.full((4 * Rh * Rw, 8), float('nan'), device=dev, dtype=torch.bfloat16)
        args = (b['image_raw'].to(dev), off.to(dev), hw.to(dev))
        if augment:
            ops.image_ingest_aug(*args, b['image_aug'].to(dev), Rh, Rw, hand, 0, host=(off, hw, b['image_aug']))
        else:
            ops.image_ingest_rect(*args, Rh, Rw, hand, 0, host=(off, hw))
        fed = model.ingest_raw(b)
        assert not any(k in fed for k in ('image_raw', 'image_off', 'image_hw', 'image_size', 'image_aug'))
        assert fed['image_nhwc8'].shape == (4, Rh, Rw, 8)
        assert torch.equal(_bits(fed['image_nhwc8'].reshape(-1, 8)), _bits(hand))
        seen.add((Rh, Rw))
    assert len(seen) == 4


def _step(model, batch, dev, seed):
    """loss and a copy of the flat gradient of one forward / backward of a raw batch, as ``Trainer.fit`` feeds it"""
    if 'image_raw' in batch:
        batch = model.ingest_raw(batch)
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}
    torch.manual_seed(seed)            # the VAE's sample, the timesteps and the noise
    torch.cuda.manual_seed_all(seed)
    model.unet.zero_grad()
    out = model(batch)
    loss = model.loss(out, batch)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), model.unet.grad.clone(), tuple(out[0].shape)


def test_a_step_per_bucket_shape_equals_the_single_shape_rectangular_path(image_dir, model, dev):
    """For the first batch of every bucket, in the order the epoch brings them (so the shape changes from step to step):
    loss and flat gradient of the bucketed batch against the same samples collated by hand for that one ``(Rh, Rw)`` -
    the path rectangular training already takes.  Then the first shape once more: it gives what it gave before the others
    ran (scratch and workspaces are rebuilt per shape, not left over from the last one)."""
    from diffusion_amd.datasets.image_ingest import collate_raw_images
    dl = _loader(image_dir)
    dl.set_epoch(0)
    batches = list(dl)
    dl.batch_sampler.set_epoch(0)
    indices = list(dl.batch_sampler)
    assert len(batches) == len(indices) == 10
    inner = dl.dataset.dataset   # the samples without their bucket: what a single-shape run reads
    first, done = None, {}
    for k, (b, idx) in enumerate(zip(batches, indices)):
        shape = b['image_size']
        if shape in done:
            continue
        loss, grad, oshape = _step(model, dict(b), dev, 100 + k)
        assert oshape == (4, 4, shape[0] // 8, shape[1] // 8)
        hand = collate_raw_images(image_size=shape)([inner[i] for i in idx])
        assert hand['image_size'] == shape and torch.equal(hand['image_hw'], b['image_hw'])
        loss2, grad2, _ = _step(model, hand, dev, 100 + k)
        assert torch.isfinite(loss).item() and loss.item() > 0 and float(grad.abs().sum()) > 0
        assert torch.equal(loss, loss2), (shape, loss.item(), loss2.item())
        assert torch.equal(grad, grad2), shape
        done[shape] = (k, loss, grad)
        first = first or shape
    assert len(done) == 4
    k, loss, grad = done[first]
    again = _step(model, dict(batches[k]), dev, 100 + k)
    assert torch.equal(again[0], loss) and torch.equal(again[1], grad)


def _cfg(image_dir, folder, *extra):
    from diffusion_amd import hydra_lite as h
    return h.load_config(YAML, [
        'batch_size=4', 'model.model_name=tiny', 'model.precomputed_latents=false', 'trainer.device_train_microbatch_size=auto',
        f'dataset.train_dataset.local={image_dir}', 'dataset.train_dataset.resize_size=128',
        'dataset.train_dataset.aspect_buckets={step: 64, min_side: 64, max_side: 256}', 'dataset.train_dataset.random_crop=true',
        'dataset.train_dataset.flip_prob=0.5', 'dataset.train_dataset.num_workers=0', 'optimizer.lr=1.0e-3', 'scheduler.t_warmup=0ba',
        'trainer.log_every=1', f'trainer.save_folder={folder}', 'trainer.save_interval=3ba'] + list(extra))


def _losses(tr):
    return {d['batch']: d['loss/train/total'] for d in tr.logs if 'loss/train/total' in d}


def test_bucketed_run_is_repeatable_and_resumes_mid_epoch_bit_for_bit(image_dir, dev, tmp_path):
    """Six steps from the shipped bucket config (tiny model, raw images, ``random_crop`` and ``flip_prob=0.5`` on) twice: the
    same losses.  Three steps, a checkpoint, and a fresh Trainer resumed to six: steps 4-6 and the weights of the uninterrupted
    run - the sampler's ``skip``, the draws of (seed, epoch, index) and the restored RNG streams reproduce the data."""
    from diffusion_amd.train import train
    full = train(_cfg(image_dir, tmp_path / 'a', 'trainer.max_duration=6ba'))
    shapes = {s for s in full._auto_mb}
    assert len(shapes) >= 2, shapes            # the run did alternate shapes; auto_microbatch was resolved per shape
    twin = train(_cfg(image_dir, tmp_path / 'b', 'trainer.max_duration=6ba'))
    lf, lt = _losses(full), _losses(twin)
    assert sorted(lf) == [1, 2, 3, 4, 5, 6] and lf == lt, (lf, lt)
    assert all(np.isfinite(v) and v > 0 for v in lf.values())
    ck = os.path.join(tmp_path, 'a', 'ba3-rank0.pt')
    torch.manual_seed(999)            # a resumed process starts from unrelated generator states
    torch.cuda.manual_seed_all(999)
    res = train(_cfg(image_dir, tmp_path / 'c', 'trainer.max_duration=6ba', f'trainer.load_path={ck}'))
    lr = _losses(res)
    assert res.batch_idx == 6 and sorted(lr) == [4, 5, 6]
    for b in (4, 5, 6):
        assert lf[b] == lr[b], (b, lf[b], lr[b])
    assert torch.equal(full.model.unet.master, res.model.unet.master)


@pytest.fixture(scope='module')
def latent_dir(image_dir, dev, tmp_path_factory):
    """tools/precompute_latents.py --aspect-buckets 128 on the image directory, with the tool's tiny encoders"""
    spec = importlib.util.spec_from_file_location('precompute_latents', os.path.join(ROOT, 'tools', 'precompute_latents.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = str(tmp_path_factory.mktemp('buckets_lat') / 'lat')
    enc = tool.build_encoders('tiny', seed=17)
    res = tool.precompute(image_dir, out, resolutions=(32,), batch_size=8, seed=17, caption_drop_prob=0.0, encoders=enc,
                          aspect_buckets=128, bucket_step=64, bucket_min=64, bucket_max=256)
    assert res['images'] == 40
    return out, enc


def test_precompute_writes_each_image_encoded_at_its_bucket(image_dir, latent_dir, dev):
    """every ``latents_ar128`` is ``sample() * 0.18215`` (fp16) of the HIP VAE encoder on the rectangular ingest of that image
    at its bucket, recomputed here batch by batch as the tool groups them (batches of 8 in disk order, buckets in table order,
    the bucketed columns' own generator); ``latents_ar128_hw`` is the bucket; what the tool wrote before is still there"""
    from diffusion_amd import ops
    from diffusion_amd.datasets.buckets import assign_bucket
    from diffusion_amd.datasets.image_ingest import decode_rgb, pack_images
    from diffusion_amd.datasets.mds import MDSDirectory
    from diffusion_amd.models.vae import DiagonalGaussian
    out_dir, enc = latent_dir
    src, out = MDSDirectory(image_dir), MDSDirectory(out_dir)
    assert len(out) == 40
    gen = torch.Generator(device='cuda').manual_seed(17 + 1)
    for b0 in range(0, 40, 8):
        imgs = [torch.from_numpy(decode_rgb(src.get(i, columns=('jpg',))['jpg'])) for i in range(b0, b0 + 8)]
        which = [assign_bucket(im.shape[1], im.shape[0], T5) for im in imgs]
        for bi in sorted(set(which)):
            sel = [j for j, w in enumerate(which) if w == bi]
            Rh, Rw = T5[bi]
            raw, off, hw = pack_images([imgs[j] for j in sel])
            x = torch.empty(len(sel) * Rh * Rw, 8, device=dev, dtype=torch.bfloat16)
            ops.image_ingest_rect(raw.to(dev), off.to(dev), hw.to(dev), Rh, Rw, x, 0, host=(off, hw))
            want = (DiagonalGaussian(enc[0].moments_nhwc8(x, len(sel), Rh, Rw)).sample(generator=gen) * 0.18215).half().cpu()
            for n, j in enumerate(sel):
                got = out.get(b0 + j)
                assert set(got) == {'jpg', 'caption', 'caption_latents', 'latents_32', 'latents_ar128', 'latents_ar128_hw'}
                assert np.frombuffer(got['latents_ar128_hw'], np.int32).tolist() == [Rh, Rw]
                stored = torch.from_numpy(np.frombuffer(got['latents_ar128'], np.float16).copy()).view(4, Rh // 8, Rw // 8)
                assert torch.equal(stored, want[n]), (b0 + j, (Rh, Rw))
                assert got['jpg'] == src.get(b0 + j)['jpg'] and len(got['latents_32']) in (0, 4 * 4 * 4 * 2)


def test_training_from_bucketed_latents_sees_their_shapes_and_graph_replay_equals_eager(latent_dir, dev):
    """the latent directory through the dataloader: every batch has the shape of its ``_hw`` column; six Trainer steps over
    the alternating shapes give the same losses and weights eagerly and with every microbatch replayed from a graph captured
    per shape"""
    from diffusion_amd.datasets.laion.laion import build_streaming_laion_dataloader
    from diffusion_amd.models.models import stable_diffusion_2
    from diffusion_amd.optim import FusedAdamW
    from diffusion_amd.trainer import Trainer
    out_dir, _ = latent_dir

    def loader():
        return build_streaming_laion_dataloader(local=out_dir, batch_size=4, resize_size=128, aspect_buckets=True, seed=11)

    dl = loader()
    assert dl.bucket_table == [t for t in T5 if t != (256, 64)]
    shapes = [tuple(b['image_latents'].shape) for b in dl]
    assert len(shapes) == 10 and {s[2:] for s in shapes} == {(Rh // 8, Rw // 8) for Rh, Rw in dl.bucket_table}
    assert all(s[:2] == (4, 4) for s in shapes)

    def run(use_graphs):
        torch.manual_seed(21)
        torch.cuda.manual_seed_all(21)
        m = stable_diffusion_2(model_name='tiny', pretrained=False, precomputed_latents=True, fsdp=False, seed=3)
        tr = Trainer(m, train_dataloader=loader(), optimizers=FusedAdamW(lr=1e-3, weight_decay=0.01, unet=m.unet),
                     max_duration='6ba', device_train_microbatch_size=4, use_graphs=use_graphs, log_every=1)
        tr.fit()
        torch.cuda.synchronize()
        return tr

    eager, graphed = run(False), run(True)
    le, lg = _losses(eager), _losses(graphed)
    assert sorted(le) == [1, 2, 3, 4, 5, 6] and le == lg, (le, lg)
    assert torch.equal(eager.model.unet.master, graphed.model.unet.master)
    n_shapes = len({s for s in shapes[:6]})
    assert n_shapes >= 2 and graphed._graph_cache.captures == len(graphed._graph_cache.graphs) == n_shapes
    assert eager._graph_cache is None or not eager._graph_cache.graphs

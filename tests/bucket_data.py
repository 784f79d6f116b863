"""The 40-image MDS directory the aspect-ratio bucketing tests share (tests/test_buckets_host.py, tests/test_buckets_gpu.py):
four aspect ratios that land in four of the five buckets of ``bucket_table(128, 64, 64, 256)``, 8 to 12 images each, every
image of another size (so ``(h, w)`` names a sample), interleaved on disk and spread over three shards."""
import io

import numpy as np

from ingest_reference import seeded_image

T5 = [(64, 192), (64, 256), (128, 128), (192, 64), (256, 64)]
BUCKET_KW = dict(step=64, min_side=64, max_side=256)

# (h, w): 3:1 -> (64, 192); a little over 4:1 -> (64, 256); square -> (128, 128); 1:3 -> (192, 64)
SHAPES = [(20 + i, 3 * (20 + i)) for i in range(8)] + [(12 + i, 4 * (12 + i) + 3) for i in range(12)] \
    + [(30 + i, 30 + i) for i in range(12)] + [(3 * (16 + i), 16 + i) for i in range(8)]
ORDER = np.random.default_rng(5).permutation(len(SHAPES)).tolist()   # sample k on disk is SHAPES[ORDER[k]]


def png(arr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format='PNG')
    return buf.getvalue()


def image(k):
    """the pixels of sample k on disk"""
    return seeded_image(*SHAPES[ORDER[k]], 500 + ORDER[k])


def write_image_mds(directory):
    from diffusion_amd.datasets.mds import write_mds
    smp = [{'jpg': png(image(k)), 'caption': f'image {ORDER[k]}'} for k in range(len(ORDER))]
    write_mds(directory, {'jpg': 'bytes', 'caption': 'str'}, smp, samples_per_shard=16)
    return directory

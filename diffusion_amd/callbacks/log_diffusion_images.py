"""Images generated from fixed prompts during evaluation - the reference's diffusion/callbacks/log_diffusion_images.py
without W&B: the images are written as PNG files and their paths logged."""
from __future__ import annotations

import os
from typing import List, Optional

import torch

from ..trainer import Callback


class LogDiffusionImages(Callback):
    """On the first batch of every ``Trainer.eval()``: generate one image per prompt and write it to
    ``<trainer.save_folder or '.'>/images/ba<batch_idx>/<k>.png`` (rank 0 only), logging ``{'images/<prompt>': path}``
    through ``trainer.log``.  The prompts are tokenized once, with the model's tokenizer.

    Args (log_diffusion_images.py:36-43):
        prompts (List[str]): the prompts.
        size (int, optional): side of the generated images. Default: ``256``.
        num_inference_steps (int, optional): sampler steps. Default: ``50``.
        guidance_scale (float, optional): classifier-free guidance weight, enabled above 1. Default: ``0.0``.
        text_key (str, optional): the batch's key of the tokenized captions. Default: ``'captions'``.
        tokenized_prompts (torch.LongTensor, optional): pre-tokenized prompts to use instead. Default: ``None``.
        seed (int, optional): seed of the generation. Default: ``1138``.
    """

    def __init__(self, prompts: List[str], size: Optional[int] = 256, num_inference_steps=50,
                 guidance_scale: Optional[float] = 0.0, text_key: Optional[str] = 'captions',
                 tokenized_prompts: Optional[torch.LongTensor] = None, seed: Optional[int] = 1138):
        self.prompts, self.size, self.num_inference_steps = list(prompts), size, num_inference_steps
        self.guidance_scale, self.text_key, self.seed = guidance_scale, text_key, seed
        self.tokenized_prompts = tokenized_prompts

    def eval_batch_end(self, trainer, batch, outputs, index):
        if index != 0:   # once per evaluation
            return
        model = trainer.model
        if self.tokenized_prompts is None:   # once, for all evaluations
            self.tokenized_prompts = model.tokenizer(self.prompts, padding='max_length', truncation=True,
                                                     return_tensors='pt')['input_ids']
        self.tokenized_prompts = self.tokenized_prompts.to(batch[self.text_key].device)
        gen_images = model.generate(tokenized_prompts=self.tokenized_prompts, height=self.size, width=self.size,
                                    guidance_scale=self.guidance_scale, progress_bar=False,
                                    num_inference_steps=self.num_inference_steps, seed=self.seed)
        if trainer.rank != 0:
            return
        from PIL import Image
        folder = os.path.join(trainer.save_folder or '.', 'images', f'ba{trainer.batch_idx}')
        os.makedirs(folder, exist_ok=True)
        u8 = (gen_images.float().clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
        logged = {}
        for k, (prompt, image) in enumerate(zip(self.prompts, u8)):
            path = os.path.join(folder, f'{k}.png')
            Image.fromarray(image).save(path)
            logged[f'images/{prompt}'] = path
        trainer.log(logged)

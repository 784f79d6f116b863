"""Child process of tests/test_grad_norm_gpu.py (not collected by pytest): two clipped optimizer steps of the tiny-width
model on this rank's half of a fixed global batch, through Trainer.train_batch with GradientClipping on.

  python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 tests/grad_norm_dp_worker.py OUT
  (DA_DIST_BACKEND=gloo lets the ranks share one GPU; DA_DP_COLLECTIVE / DA_DP_PAYLOAD select the exchange)
Every rank writes OUT.rank<r>.pt: the device record after each step and the master weights before / after."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffusion_amd  # noqa: E402,F401  (sets HSA_ENABLE_IPC_MODE_LEGACY=0 before the HIP runtime starts)
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

GLOBAL_BATCH, S, CTX, STEPS = 8, 16, 128, 2
THRESHOLD = 1e-3   # far under the norm of a freshly initialised model's gradient: the clip bites (the test checks it did)


def main():
    out = sys.argv[1]
    from diffusion_amd.parallel import init_distributed_from_env
    rank, local, world = init_distributed_from_env(device_index=0)
    dev = torch.device('cuda', torch.cuda.current_device())
    from diffusion_amd.algorithms.gradient_clipping import GradientClipping
    from diffusion_amd.models.models import stable_diffusion_2
    from diffusion_amd.optim import FusedAdamW
    from diffusion_amd.trainer import Trainer
    model = stable_diffusion_2(model_name='tiny', pretrained=False, precomputed_latents=True, fsdp=False, seed=3)
    opt = FusedAdamW(lr=1e-3, weight_decay=0.01, unet=model.unet)
    tr = Trainer(model, train_dataloader=None, optimizers=opt, max_duration=f'{STEPS}ba',
                 algorithms=[GradientClipping('norm', THRESHOLD)])
    tr.reducer.bucket = 1_000_000          # several buckets at tiny width
    before = model.unet.master.detach().cpu().clone()
    g = torch.Generator().manual_seed(11)
    per = GLOBAL_BATCH // world
    stats = []
    for _ in range(STEPS):
        full = {'image_latents': torch.randn(GLOBAL_BATCH, 4, S, S, generator=g).half(),
                'caption_latents': torch.randn(GLOBAL_BATCH, 77, CTX, generator=g).half(),
                '_noise': torch.randn(GLOBAL_BATCH, 4, S, S, generator=g),
                '_timesteps': torch.randint(0, 1000, (GLOBAL_BATCH,), generator=g)}
        tr.train_batch({k: v[rank * per:(rank + 1) * per].to(dev) for k, v in full.items()})
        tr.batch_idx += 1
        torch.cuda.synchronize()
        stats.append(opt._gn['stats'].detach().cpu().clone())
    torch.save({'stats': stats, 'before': before, 'master': model.unet.master.detach().cpu().clone(), 'world': world,
                'reducer_enabled': tr.reducer.enabled, 'sliced': tr.sliced_optimizer}, f'{out}.rank{rank}.pt')
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()

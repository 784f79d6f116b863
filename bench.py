"""bench.py - U-Net training throughput (images/sec) of the SD-2-base training step on MI355X.

  python bench.py --gpus N --steps K --warmup W            (N=1 default)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \\
         bench.py --gpus N --steps K --warmup W            (one rank per GPU, RCCL)

A "step" = one optimizer step over the per-GPU batch (BASELINE.json configs[1]: SD-2-base U-Net only, precomputed
latents 4x32x32, batch 256 per GPU, bf16): forward + fused MSE + backward of the 865.9 M-parameter U-Net, gradient
all-reduce over RCCL (N>1) overlapped with the backward, fused AdamW.  Weak scaling: the per-GPU batch is fixed, global
batch = 256*N (2048 at N=8 = the reference's configuration).  Inputs (fp16 latents and text embeddings, as the reference
dataloader yields them) are resident in HBM before the timed region; timestep and noise draws are inside it, as in the
reference's forward.  Weights are torch-default random init (seed 17).

Prints ONE JSON line on rank 0.  `value` and `ms_per_step` come from an UN-INSTRUMENTED timed loop; a plain run does
nothing else.  With --full the line also carries: `roofline` (the dominant kernel: the 256x320-tile, 16-wave
implicit-GEMM gemm_nt2_kernel<4,5,4,4>, conv / linear forward + dgrad) and `kernels` from a second short loop with HIP
events around every launch; `secondary`, the 512-px row of the metric (latents 4x64x64, batch 64 per GPU) measured in the
same process; `cpu_baseline`, the oracle port on the host cores (N=1 only).

--dump-outputs DIR writes what the last timed step computed, on rank 0, before anything else runs: `loss.npy` (float64,
the step's loss) and a fixed sample (DUMP_SAMPLE offsets drawn with seed DUMP_SEED) of the flat fp32 gradient and of
the updated fp32 master weights (`grad_sample.npy`, `master_sample.npy`, float32, 16 MiB each).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# importing the package puts HSA_ENABLE_IPC_MODE_LEGACY=0 into the environment (diffusion_amd/__init__.py: the one place
# run.py, bench.py and the tests share) before torch can start the HIP runtime
import diffusion_amd  # noqa: E402,F401
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

TRAIN_GFLOP_PER_IMG = {32: 543.27, 64: 2412.77, 96: 6447.32}  # fwd+dgrad+wgrad, 2*MAC
PROFILE_STEPS = 2      # instrumented steps behind `roofline` / `kernels` (outside the timed region)
SECONDARY_STEPS = 5    # timed steps of the 512-px secondary block
PEAK_BF16_TFLOPS = 2500.0  # dense MFMA bf16 peak, /opt/skills/guides/MI355X_MICROARCH.md
README_8xA100 = {32: 1100.0, 64: 290.0}  # /root/reference README.md:56 (8xA100, global batch 2048)
DUMP_SAMPLE = 1 << 22  # flat offsets sampled by --dump-outputs (with replacement, sorted)
DUMP_SEED = 0


def _usable_cores():
    """Cores this process may actually use: the affinity mask capped by the cgroup CPU quota (a GPU box hands a 1-GPU
    job a share of the host, and 128 threads on a 16-core share only thrash)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    try:
        with open('/sys/fs/cgroup/cpu.max') as f:
            quota, period = f.read().split()
        if quota != 'max':
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, n)


def cpu_baseline(seconds_budget=30.0):
    """Oracle (CPU port of the same training step, fp32) on the host cores.

    BASELINE.json configs[0] is batch 4, one process; a whole batch-4 step costs ~45 s of CPU on the GPU box, so the
    default is a stated TIME-BOXED SUBSET of it: per-image cost of this path does not depend on the batch (every op is a
    per-image GEMM / conv), so steps are run at batch 1 - one untimed warm-up step, then timed steps (forward, backward,
    AdamW over all 686 parameter tensors) until the budget is spent (at most 3), median reported.  BENCH_CPU_FULL=1 runs
    cfg 1 as written instead (batch 4, 1 warm-up + median of 3)."""
    from oracle import unet_oracle as O
    cfg = O.UNetConfig.sd2_base()
    torch.set_num_threads(_usable_cores())
    torch.manual_seed(17)
    sd = {}
    for k, shape in O.param_manifest(cfg):  # fast init: statistics as init_state_dict, cheaper RNG
        if 'norm' in k.rsplit('.', 2)[-2]:
            sd[k] = torch.ones(shape) if k.endswith('weight') else torch.zeros(shape)
        else:
            fan = max(1, int(torch.tensor(shape[1:]).prod().item())) if len(shape) > 1 else shape[0]
            sd[k] = (torch.rand(shape) * 2 - 1) / fan**0.5
    full = os.environ.get('BENCH_CPU_FULL') == '1'
    B, S = (4 if full else 1), 32
    g = torch.Generator().manual_seed(17)
    lat = torch.randn(B, 4, S, S, generator=g)
    ctx = torch.randn(B, 77, 1024, generator=g)
    noise = torch.randn(B, 4, S, S, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    m = {k: torch.zeros_like(v) for k, v in sd.items()}
    v = {k: torch.zeros_like(v) for k, v in sd.items()}

    def step(i):
        t0 = time.perf_counter()
        _, _, grads = O.training_loss_and_grads(sd, cfg, lat, t, ctx, noise)
        with torch.no_grad():
            for k in sd:
                sd[k], m[k], v[k] = O.adamw_step(sd[k], grads[k], m[k], v[k], i, 1e-4)
        return time.perf_counter() - t0

    t_all = time.perf_counter()
    warm = step(1)
    times = []
    while len(times) < 3:
        times.append(step(2 + len(times)))
        if not full and (time.perf_counter() - t_all) + times[-1] > seconds_budget:
            break
    med = sorted(times)[len(times) // 2]
    return {'value': round(B / med, 4), 'unit': 'images/sec', 'cores': torch.get_num_threads(), 'kind': 'port',
            'sample': (f'oracle/unet_oracle.py, fp32, SD-2-base U-Net train step (fwd + bwd + AdamW on all 686 tensors), '
                       f'4x32x32 latents, batch {B}: 1 warm-up step ({warm:.1f} s) + median of {len(times)} timed step(s) '
                       f'({med:.1f} s each)' + ('' if full else '; time-boxed subset of cfg 1 (batch 4) - per-image '
                                                'cost is batch-independent on this path'))}


def kernel_table(prof):
    """ops.PROFILE (HIP events around every launch, on the launch stream) -> per-kernel {launches, ms, avg_us, tflops},
    the dominant implicit-GEMM kernel and its roofline block."""
    prof = dict(prof)
    shapes = prof.pop('_shapes', [])
    kern = {}
    for k, evs in prof.items():
        ms = sum(s.elapsed_time(e) for s, e, _ in evs)
        fl = sum(f for _, _, f in evs)
        kern[k] = {'launches': len(evs), 'ms': round(ms, 2), 'avg_us': round(1000 * ms / len(evs), 2),
                   'tflops': round(fl / ms / 1e9, 1) if ms > 0 else None}
    if 'attn_bwd' in kern and kern['attn_bwd']['tflops']:
        # counted as 2 x forward (four N x N x 64 products), consistent with SURVEY 8(d)'s train = 3 x fwd; the
        # FlashAttention convention counts the recomputed S as well (five products, 2.5 x forward)
        kern['attn_bwd']['flops_convention'] = '8*B*H*Nq*Nk*64 (2 x forward)'
        kern['attn_bwd']['tflops_5_products'] = round(kern['attn_bwd']['tflops'] * 1.25, 1)
    dom = max((k for k in kern if k.startswith('gemm_nt')), key=lambda k: kern[k]['ms'])
    gk = kern[dom]
    roof = {'bound': 'mfma', 'kernel': dom, 'profiled_steps': PROFILE_STEPS, 'achieved': gk['tflops'],
            'peak': PEAK_BF16_TFLOPS, 'unit': 'TFLOP/s', 'frac': round(gk['tflops'] / PEAK_BF16_TFLOPS, 4),
            'avg_launch_us': gk['avg_us'], 'launches': gk['launches'], 'traffic': None}
    return kern, dom, roof, shapes


def dump_outputs(out_dir, loss, unet):
    """--dump-outputs: the last timed step's loss and a seeded sample of its gradient and updated weights, as .npy."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    g = torch.Generator().manual_seed(DUMP_SEED)
    idx = torch.randint(0, unet.master.numel(), (DUMP_SAMPLE,), generator=g).sort().values.to(unet.master.device)
    np.save(os.path.join(out_dir, 'loss.npy'), np.array([loss], dtype=np.float64))
    np.save(os.path.join(out_dir, 'grad_sample.npy'), unet.grad[idx].cpu().numpy())
    np.save(os.path.join(out_dir, 'master_sample.npy'), unet.master[idx].cpu().numpy())


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        return sk.getsockname()[1]


def spawn_ranks(n: int) -> int:
    """`python bench.py --gpus N` without a torchrun environment: start the N ranks ourselves, the way the reference's
    `composer run.py` spawns its own (README.md:86-93, sensecore/run_cmd.sh:23-33).  The parent makes NO GPU call (it
    never touches torch.cuda), relays the children's output - rank 0 prints the one JSON line - and returns their status."""
    import subprocess
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={n}',
           '--master-addr', '127.0.0.1', '--master-port', str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault('OMP_NUM_THREADS', str(max(1, _usable_cores() // n)))
    return subprocess.run(cmd, env=env).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=4)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--latent', type=int, default=32, help='latent side: 32 (256 px), 64 (512 px), 96 (768 px v-pred)')
    ap.add_argument('--batch', type=int, default=None, help='per-GPU batch (default 256 @32, 64 @64, 16 @96)')
    ap.add_argument('--microbatch', type=int, default=None)
    ap.add_argument('--full', action='store_true',
                    help='after the timed steps also run the per-kernel timing loop, the 512-px secondary block and the '
                         'CPU baseline (each can be left out with its --no-* option)')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-kernel-timing', action='store_true')
    ap.add_argument('--no-secondary', action='store_true', help='skip the 512-px secondary block')
    ap.add_argument('--full-pipeline', action='store_true',
                    help='BASELINE cfg 3: precomputed_latents=false - frozen VAE-encode + CLIP text-encode on PyTorch-ROCm '
                         '(random-init fp16 encoders, synthetic images / token ids) inside the timed step')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write the last timed step\'s loss, gradient and weight samples to DIR/*.npy')
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error('--steps must be >= 1 and --warmup >= 0')

    if a.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        raise SystemExit(spawn_ranks(a.gpus))
    from diffusion_amd.parallel import init_distributed_from_env
    rank, local, world = init_distributed_from_env()
    if world != a.gpus:
        raise SystemExit(f'--gpus {a.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {a.gpus}')
    dev = torch.device('cuda', torch.cuda.current_device())

    from diffusion_amd import ops
    from diffusion_amd.models.models import stable_diffusion_2
    from diffusion_amd.optim import FusedAdamW
    from diffusion_amd.trainer import Trainer

    S = a.latent
    B = a.batch or {32: 256, 64: 64, 96: 16}[S]
    mb = a.microbatch or {32: 256, 64: 64, 96: 16}[S]
    name = 'stabilityai/stable-diffusion-2' if S == 96 else 'stabilityai/stable-diffusion-2-base'
    torch.manual_seed(17 + rank)
    model = stable_diffusion_2(model_name=name, pretrained=False, precomputed_latents=not a.full_pipeline, fsdp=False,
                               seed=17)
    opt = FusedAdamW(lr=1e-4, weight_decay=0.01, unet=model.unet)
    trainer = Trainer(model, train_dataloader=None, optimizers=opt, max_duration='1ba', device_train_microbatch_size=mb)
    g = torch.Generator().manual_seed(1000 + rank)
    if a.full_pipeline:
        batch = {'image': (torch.rand(B, 3, 8 * S, 8 * S, generator=g) * 2 - 1).to(dev),
                 'captions': torch.randint(0, 49408, (B, 77), generator=g).to(dev)}
    else:
        batch = {'image_latents': torch.randn(B, 4, S, S, generator=g).half().to(dev),
                 'caption_latents': torch.randn(B, 77, 1024, generator=g).half().to(dev)}

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(bt, steps, warmup):
        """W untimed steps, then EXACTLY `steps` steps between barrier + synchronize pairs; max over ranks."""
        ls = None
        for _ in range(warmup):
            ls = trainer.train_batch(bt)
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            ls = trainer.train_batch(bt)
        sync()
        el = time.perf_counter() - t0
        tm = torch.tensor([el], device=dev, dtype=torch.float64)
        if world > 1:
            dist.all_reduce(tm, op=dist.ReduceOp.MAX)
        return float(tm.item()), float(ls.item())

    # (1) the measured value: no per-kernel instrumentation inside the timed region
    dt, lossv = timed(batch, a.steps, a.warmup)
    if a.dump_outputs and rank == 0:   # before any further step changes the gradient and the weights
        dump_outputs(a.dump_outputs, lossv, model.unet)
    # (2) per-kernel timings (HIP events around every launch, on the launch stream) from a second, short loop
    prof = None
    if a.full and not a.no_kernel_timing:
        ops.PROFILE = {}
        for _ in range(PROFILE_STEPS):
            trainer.train_batch(batch)
        sync()
        prof, ops.PROFILE = ops.PROFILE, None
    # (3) the metric is quoted "@256 and @512": the 512-px row (latents 4x64x64, batch 64 per GPU) as a secondary block
    second = None
    if a.full and S == 32 and not a.full_pipeline and not a.no_secondary:
        B2 = 64
        g2 = torch.Generator().manual_seed(2000 + rank)
        batch2 = {'image_latents': torch.randn(B2, 4, 64, 64, generator=g2).half().to(dev),
                  'caption_latents': torch.randn(B2, 77, 1024, generator=g2).half().to(dev)}
        del batch
        trainer.microbatch = B2
        dt2, loss2 = timed(batch2, SECONDARY_STEPS, 2)
        ips2 = B2 * world * SECONDARY_STEPS / dt2
        prof2 = None
        if not a.no_kernel_timing:   # the @512 half of the metric gets the same per-kernel footing as the @256 half
            ops.PROFILE = {}
            for _ in range(PROFILE_STEPS):
                trainer.train_batch(batch2)
            sync()
            prof2, ops.PROFILE = ops.PROFILE, None
        second = {'metric': 'U-Net training images/sec @512 (SD-2-base U-Net, precomputed latents 4x64x64)',
                  'value': round(ips2, 2), 'unit': 'images/sec', 'steps': SECONDARY_STEPS, 'warmup': 2,
                  'ms_per_step': round(1000 * dt2 / SECONDARY_STEPS, 2),
                  'config': {'workload': f'SD-2-base U-Net train step, latents 4x64x64, text 77x1024, batch {B2}/GPU '
                                         f'(global {B2 * world}), microbatch {B2}, AdamW, dp{world}'},
                  'loss': round(loss2, 5),
                  'step_tflops_per_gpu': round(ips2 / world * TRAIN_GFLOP_PER_IMG[64] / 1000, 1),
                  'vs_baseline': round(ips2 / README_8xA100[64], 3) if world == 8 else None}
        if prof2:
            kern2, _, roof2, _ = kernel_table(prof2)
            second['roofline'] = roof2
            second['kernels'] = {k: kern2[k] for k in kern2 if k.startswith(('gemm_nt2_kernel<4,5,4,4>', 'gemm_nt_ws', 'gemm_tn', 'attn'))}

    if rank == 0:
        ips = B * world * a.steps / dt
        out = {
            'metric': (f'U-Net training images/sec @{S * 8} ({"SD-2.1-768-v" if S == 96 else "SD-2-base"} U-Net, ' +
                       (f'online VAE+CLIP encode, images 3x{8 * S}x{8 * S})' if a.full_pipeline else
                        f'precomputed latents 4x{S}x{S})')),
            'value': round(ips, 2), 'unit': 'images/sec', 'n_gpus': world, 'steps': a.steps, 'warmup': a.warmup,
            'ms_per_step': round(1000 * dt / a.steps, 2), 'higher_is_better': True, 'scaling': 'weak',
            'vs_baseline': (round(ips / README_8xA100[S], 3) if (world == 8 and S in README_8xA100) else None),
            'dtype': 'bf16', 'data': 'synthetic',
            'config': {'workload': f'{"SD-2.1-768-v (v-prediction)" if S == 96 else "SD-2-base"} U-Net train step, '
                                   + ('online VAE + CLIP text encode, ' if a.full_pipeline else '') +
                                   f'latents 4x{S}x{S}, text 77x1024, batch {B}/GPU '
                                   f'(global {B * world}), microbatch {mb}, AdamW, dp{world}',
                       'global_batch': B * world, 'microbatch': mb, 'parallelism': f'dp{world}',
                       'params': model.unet.num_params},
            'loss': round(lossv, 5),
            'step_tflops_per_gpu': round(ips / world * TRAIN_GFLOP_PER_IMG[S] / 1000, 1),
            'step_frac_of_mfma_peak': round(ips / world * TRAIN_GFLOP_PER_IMG[S] / 1000 / PEAK_BF16_TFLOPS, 4),
        }
        if prof:
            kern, dom, out['roofline'], shapes = kernel_table(prof)
            # HBM bytes per launch come from rocprofv3 PMC passes (FETCH_SIZE / WRITE_SIZE cannot be read from inside the
            # process); the committed summary of those passes over this same command is reported with its provenance
            import glob
            cands = sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r*_pmc_hbm_traffic.json')))
            if S == 32 and B == 256 and mb == 256 and not a.full_pipeline and cands:
                tp = cands[-1]
                with open(tp) as f:
                    pm = json.load(f)
                key = dom.replace('gemm_nt2_kernel', 'gemm_nt2')
                if key in pm:
                    out['roofline']['traffic'] = round(pm[key]['hbm_bytes_per_launch_corrected'])
                    out['roofline']['traffic_source'] = (f'profiles/{os.path.basename(tp)} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, '
                                                         'separate passes over this command; gfx950 FETCH_SIZE x2 correction)')
            out['kernels'] = kern
            if os.environ.get('BENCH_SHAPES'):
                agg = {}
                for s_, e_, f_, tag in shapes:
                    a_ = agg.setdefault(tag, [0, 0.0, 0.0])
                    a_[0] += 1; a_[1] += s_.elapsed_time(e_); a_[2] += f_
                top = sorted(agg.items(), key=lambda kv: -kv[1][1])[:40]
                for tag, (n_, ms_, fl_) in top:
                    print(f'  {str(tag):48s} n={n_:4d} ms={ms_:8.2f} TF/s={fl_ / ms_ / 1e9:7.1f}', file=sys.stderr)
        if second is not None:
            out['secondary'] = second
        if a.full and world == 1 and not a.no_cpu_baseline:
            out['cpu_baseline'] = cpu_baseline()
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()

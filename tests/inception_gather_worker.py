"""Child process of tests/test_inception_metrics_host.py (not collected by pytest): one rank of a gloo group runs
``metrics/_inception_shared.gather_rows`` on a CPU store and writes what it got.

  RANK=r WORLD_SIZE=w MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/inception_gather_worker.py OUT_PREFIX COUNTS

COUNTS is a comma-separated row count per rank.  Rank r's store has 8 rows of width 4, row i filled with 100 r + i, and
the first COUNTS[r] of them are valid.  Rank r writes OUT_PREFIX.r.pt."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def store_of(rank):
    return (100.0 * rank + torch.arange(8, dtype=torch.float32))[:, None].expand(8, 4).contiguous()


def main():
    out, counts = sys.argv[1], [int(c) for c in sys.argv[2].split(',')]
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from diffusion_amd.metrics._inception_shared import gather_rows
    got = gather_rows(store_of(rank), counts[rank])
    torch.save(got, f'{out}.{rank}.pt')
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()

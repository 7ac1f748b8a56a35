"""One rank of the CPU stand-in for a sharded evaluate_video_gen (tests/test_video_gen_mode_cpu.py starts two of these under gloo): reads
RANK / WORLD_SIZE / MASTER_* from the environment, runs the test's own sharded evaluation with shard=None -- the driver takes rank and
world from torch.distributed --, counts the collectives the call makes and writes its returned dict.  usage: video_gen_mode_worker_cpu.py OUT_DIR"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch
import torch.distributed as dist

from tests.test_video_gen_mode_cpu import run_shard


def main():
    out_dir = sys.argv[1]
    rank = int(os.environ["RANK"])
    dist.init_process_group(backend="gloo")
    torch.set_num_threads(1)
    mine = os.path.join(out_dir, f"out{rank}")
    os.makedirs(mine)
    n = [0]
    names = ("all_gather_object", "all_gather", "all_reduce", "broadcast", "broadcast_object_list", "gather_object", "barrier")
    real = {k: getattr(dist, k) for k in names}

    def counted(k):
        def f(*a, **kw):
            n[0] += 1
            return real[k](*a, **kw)
        return f
    for k in names:
        setattr(dist, k, counted(k))
    try:
        out, _ = run_shard(None, out_dir=mine)
    finally:
        for k in names:
            setattr(dist, k, real[k])
    torch.save(dict(out=out, collectives=n[0]), os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

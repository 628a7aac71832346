"""One gloo rank of tests/test_contrib_cpu.py's all-reduce test (CPU tensors):
    python tests/contrib_reduce_worker.py <rank> <world> <port> <out.npz>"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
N_ROWS = 6


def rank_values(rank):
    """What rank `rank` holds before the all-reduce: (sum, max, pixels, views)."""
    import torch
    g = torch.Generator().manual_seed(100 + rank)
    return (torch.rand(N_ROWS, generator=g) * 50, torch.rand(N_ROWS, generator=g),
            torch.randint(0, 1 << 40, (N_ROWS,), generator=g, dtype=torch.int64),
            torch.randint(0, 9, (N_ROWS,), generator=g, dtype=torch.int32))


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    sys.path.insert(0, os.path.dirname(HERE))
    import numpy as np
    import torch.distributed as dist
    import __graft_entry__ as ge
    pkg = ge.load_package()
    dist.init_process_group("gloo", rank=rank, world_size=world, init_method=f"tcp://127.0.0.1:{port}")
    st = pkg.ContributionStats(N_ROWS, "cpu")
    for t, v in zip((st.weight_sum, st.weight_max, st.pixels, st.views), rank_values(rank)):
        t.copy_(v)
    st.all_reduce(dist)
    np.savez(out, weight_sum=st.weight_sum.numpy(), weight_max=st.weight_max.numpy(), pixels=st.pixels.numpy(),
             views=st.views.numpy())
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

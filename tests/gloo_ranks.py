"""Spawn-and-collect scaffolding of the gloo (CPU) multi-process tests —
TEST INFRASTRUCTURE ONLY.

``run_ranks(body, world, *args)`` starts ``world`` processes.  Each joins a
gloo group of that size on a port no earlier call used and runs
``body(rank, world, *args)``; ``body`` must be a module-level function (it
is pickled by name for the spawned processes).  A rank's exception
reaches the calling test as an AssertionError that carries the message of
every rank that failed.
"""

import os

import torch.distributed as dist
import torch.multiprocessing as mp

# one counter for all test modules: two groups never share a rendezvous
# port.  The single-process tests bind fixed ports below this range.
_PORT = [29900]


def _rank_main(rank, world, port, fail_q, body, args):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        body(rank, world, *args)
        dist.destroy_process_group()
    except Exception as e:  # surface the real failure to the parent
        fail_q.put(f"rank {rank}: {type(e).__name__}: {e}")
        raise


def run_ranks(body, world, *args, what="ring"):
    _PORT[0] += 1
    fail_q = mp.get_context("spawn").SimpleQueue()
    try:
        mp.spawn(
            _rank_main,
            args=(world, _PORT[0], fail_q, body, args),
            nprocs=world,
            join=True,
        )
    except Exception:
        msgs = []
        while not fail_q.empty():
            msgs.append(fail_q.get())
        raise AssertionError(f"{what} test failed:\n" + "\n".join(msgs))

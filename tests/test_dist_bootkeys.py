"""World-size-2 gloo test (CPU) of dist.broadcast_bootstrap_keys: the record
count, then each record through broadcast_bundle; every other rank receives
the records in order and byte-identical, and every rank gets the total size."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from orion_amd import dist as odist

SIZES = (1, 256, 3 << 20)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _record(i):
    return np.random.default_rng(1000 + i).integers(0, 256, SIZES[i], dtype=np.uint8)


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        got, calls = [], {"count": 0, "export": []}

        def count():
            calls["count"] += 1
            return len(SIZES)

        def export(i):
            calls["export"].append(i)
            return torch.from_numpy(_record(i))

        def load(buf):
            got.append(buf.numpy().copy())

        total = odist.broadcast_bootstrap_keys(dist, count, export, load, torch.device("cpu"))
        if rank == 0:  # the source exports each record once, in order, and imports nothing
            ok = calls == {"count": 1, "export": [0, 1, 2]} and not got
        else:
            ok = calls == {"count": 0, "export": []} and len(got) == len(SIZES) and all(
                np.array_equal(g, _record(i)) for i, g in enumerate(got))
        q.put((rank, ok, total))
    finally:
        dist.destroy_process_group()


def test_bootstrap_key_records_broadcast_world2():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert [r[0] for r in res] == [0, 1]
    assert all(r[1] for r in res), "records differ, are out of order, or the callbacks ran on the wrong rank"
    assert all(r[2] == sum(SIZES) for r in res)

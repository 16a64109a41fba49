"""What the multi-process tests share: a world of spawned rank processes that report through a queue (plain helpers, no fixtures).

A worker is ``worker(rank, world, port, *args, q)``: it joins the gloo world at 127.0.0.1:``port`` and puts ONE result into ``q`` -
a dict through ``ship`` when it carries tensors."""
import queue
import socket
import time

import numpy as np
import torch
import torch.multiprocessing as mp


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def ship(res):
    """tensors leave a worker as numpy arrays, pickled BY VALUE: a torch tensor in a multiprocessing queue travels as a file
    descriptor the parent has to fetch from the worker's resource-sharer socket - gone if the worker has exited by then
    (seen once on a GPU box: FileNotFoundError in rebuild_storage_fd)"""
    return {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in res.items()}


def collect(procs, q, world, timeout=600):
    """one result per rank (the arrays of a shipped dict as tensors again); a rank that dies (exception in the worker) fails the
    test at once instead of letting the parent sit in q.get until the timeout"""
    results, t0 = [], time.time()
    while len(results) < world:
        try:
            got = q.get(timeout=2)
            if isinstance(got, dict):
                got = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in got.items()}
            results.append(got)
        except queue.Empty:
            dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
            assert not dead, f"worker process exited with {dead}"
            assert time.time() - t0 < timeout, "timed out waiting for the ranks"
    return results


def run_world(worker, world, *args, timeout=600, join=60):
    """spawn ``world`` processes of ``worker(rank, world, port, *args, q)``, collect one result per rank, join the processes and
    check that every one exited with 0; returns the results in arrival order"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=worker, args=(r, world, port, *args, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = collect(procs, q, world, timeout)
    for p in procs:
        p.join(join)
        assert p.exitcode == 0
    return results

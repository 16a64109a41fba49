"""What the multi-process tests share: a world of spawned rank processes that report through a queue (plain helpers, no fixtures).

A worker is ``worker(rank, world, port, *args, q)``: it joins the gloo world at 127.0.0.1:``port`` and puts ONE result into ``q`` -
a dict through ``ship`` when it carries tensors."""
import os
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


def sharded_dit_loop(rank, world, port, make_model, q, stock=False, start_step=0):
    """the body of a worker that runs the tiny sharded DiT loop: 3 DDIM steps with dynamic CFG on 3 latent frames of 8 x 12 through
    ``DistDiTDenoiser`` (world 2: the CFG halves; world 4: CFG halves x latent frames (2, 1)), on ``make_model(device)``.  Puts
    {"rank", "out", "frame_shards", "steps"} and, on rank 0, "ref" and "ref_steps": ``cogvideox.denoise`` of the same inputs in
    that process.  ``stock``: no image latents and no domain / flow features (the text-to-video transformer); ``start_step`` > 0
    also hands both loops a callback, whose (index, timestep) pairs are the "steps" """
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.set_num_threads(max(1, int(os.environ.get("LKGD_TEST_HOST_CPUS", os.cpu_count() or 8)) // world))   # the ranks share the box's host cores
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from lkgd_amd import cogvideox as pc
        from lkgd_amd.dist_run import DistDiTDenoiser
        dev = torch.device("cuda", 0)
        m = make_model(dev)
        g = torch.Generator().manual_seed(79)
        lat = torch.randn(1, 3, 16, 8, 12, generator=g).half().to(dev)
        img = (0.5 * torch.randn(1, 3, 16, 8, 12, generator=g)).half().to(dev)
        pe = torch.randn(2, 16, 4096, generator=g).half().to(dev)
        dom, flow = torch.randn(1, 1, 1000, generator=g).to(dev), torch.randn(1, 1, 1000, generator=g).to(dev)
        if stock:
            img = dom = flow = None
        steps, ref_steps = [], []

        def loop_kw(seen):
            return dict(start_step=start_step, callback=lambda i, t, x: seen.append((i, t))) if start_step else {}
        runner = DistDiTDenoiser(m, pc.CogVideoXDDIMScheduler(), world, rank, 3, cfg=True)
        out = runner.denoise(lat, img, pe, dom, flow, 3, 6.0, True, **loop_kw(steps))
        res = {"rank": rank, "out": out.float().cpu(), "frame_shards": runner.plan.frame_shards, "steps": steps}
        if rank == 0:
            res["ref"] = pc.denoise(m, pc.CogVideoXDDIMScheduler(), lat, img, pe, dom, flow, 3, 6.0, True, **loop_kw(ref_steps)).float().cpu()
            res["ref_steps"] = ref_steps
        q.put(ship(res))
    finally:
        dist.destroy_process_group()

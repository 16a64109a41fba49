"""Multi-process (world_size 2, gloo, CPU) tests of the frame-parallel host logic: shard plans, the padded uneven
all-gather of frame slices, the GroupNorm partial-sum all-reduce.  The kernels themselves are covered by -m gpu tests
(tests/test_dist_gpu.py runs the sharded UNet with two ranks on one GPU)."""
import os

import pytest
import torch
import torch.distributed as dist

from dist_support import run_world
from lkgd_amd.dist import allreduce_sums, gather_frames, make_plan, split_frames


def test_split_and_plans():
    assert split_frames(14, 4) == (4, 4, 3, 3) and split_frames(14, 2) == (7, 7) and split_frames(14, 1) == (14,)
    assert split_frames(25, 4) == (7, 6, 6, 6)
    with pytest.raises(ValueError):
        split_frames(3, 4)
    p = make_plan(8, 6, 14, cfg=True)          # CFG(2) x frames(4,4,3,3)
    assert (p.cfg_groups, p.frame_shards, p.cfg_index, p.shard_index) == (2, 4, 1, 2)
    assert p.f0 == 8 and p.f_local == 3 and p.f_max == 4
    assert p.frame_group_ranks() == [4, 5, 6, 7] and p.cfg_partner_ranks() == [2, 6]
    p = make_plan(2, 1, 14, cfg=True)          # pure CFG-parallel: no frame exchange at all
    assert p.frame_shards == 1 and p.cfg_index == 1 and p.f_local == 14
    p = make_plan(4, 3, 14, cfg=False)         # guidance off: all ranks share the frames
    assert p.cfg_groups == 1 and p.splits == (4, 4, 3, 3) and p.f0 == 11
    covered = []
    for r in range(8):
        q = make_plan(8, r, 14, True)
        covered.append((q.cfg_index, q.f0, q.f0 + q.f_local))
    assert sorted(covered) == [(0, 0, 4), (0, 4, 8), (0, 8, 11), (0, 11, 14), (1, 0, 4), (1, 4, 8), (1, 8, 11),
                               (1, 11, 14)]
    with pytest.raises(ValueError):
        make_plan(3, 0, 14, cfg=True)
    # round 6: frame slices cut at multiples of `frame_unit` (the FSM hook fuses frames 2k / 2k+1: a pair lives on one rank)
    assert split_frames(14, 4, 2) == (4, 4, 4, 2) and split_frames(14, 2, 2) == (8, 6) and split_frames(8, 4, 2) == (2, 2, 2, 2)
    assert split_frames(14, 7, 2) == (2,) * 7
    with pytest.raises(ValueError):
        split_frames(14, 8, 2)                 # more shards than pairs
    with pytest.raises(ValueError):
        split_frames(13, 2, 2)                 # an odd clip has no whole pairs
    # ... and symmetric slices for flip=True joint attention: shard i and k-1-i mirror each other frame for frame
    assert split_frames(14, 4, symmetric=True) == (4, 3, 3, 4) and split_frames(7, 3, symmetric=True) == (2, 3, 2)
    assert split_frames(6, 4, symmetric=True) == (2, 1, 1, 2) and split_frames(14, 2, symmetric=True) == (7, 7)
    with pytest.raises(ValueError):
        split_frames(5, 2, symmetric=True)
    p = make_plan(8, 7, 14, cfg=True, frame_unit=2)
    assert p.splits == (4, 4, 4, 2) and p.f0 == 12 and p.f_local == 2 and all(s % 2 == 0 for s in p.splits)
    # one frame slice (pure CFG-parallel) with several entries per rank: nothing to exchange, the tokens come back as they are
    from lkgd_amd.dist_run import ShardInfo
    sh = ShardInfo(make_plan(2, 1, 6, cfg=True), None, entries=2)
    x = torch.arange(2 * 6 * 4 * 3, dtype=torch.float32).reshape(-1, 3)
    assert sh.gather(x) is x and sh.to_pixels(x, 4) is x and sh.to_frames(x, 4) is x and (sh.b0, sh.B_total) == (2, 4)


def _worker(rank, world, port, frames, q):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.set_num_threads(max(1, int(os.environ.get("LKGD_TEST_HOST_CPUS", os.cpu_count() or 8)) // world))   # the ranks share the box's host cores
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        plan = make_plan(world, rank, frames, cfg=False)
        full = torch.arange(frames * 3 * 5, dtype=torch.float32).reshape(frames, 3, 5)
        local = full[plan.f0:plan.f0 + plan.f_local].clone()
        got = gather_frames(local, plan)
        ok = torch.equal(got, full)
        sums = torch.full((1, 32, 2), float(rank + 1))
        allreduce_sums(sums, plan)
        ok = ok and torch.equal(sums, torch.full((1, 32, 2), float(sum(range(1, world + 1)))))
        # fp16 payload, as the activations are
        h = gather_frames(local.half(), plan)
        ok = ok and torch.equal(h, full.half())
        # boundary-frame exchange for the Conv3d halo: slots 0 / f_local+1 <- neighbours' last / first frame, zero at the ends
        from lkgd_amd.dist import exchange_halo
        hb = torch.zeros(plan.f_local + 2, 3, 5)
        hb[1:plan.f_local + 1] = local
        exchange_halo(hb, plan)
        padded = torch.cat([torch.zeros(1, 3, 5), full, torch.zeros(1, 3, 5)])
        ok = ok and torch.equal(hb, padded[plan.f0:plan.f0 + plan.f_local + 2])
        # both forms of the exchange (default all-gather of boundary frames, opt-in neighbour-only P2P) give the same buffer,
        # also as recorded steps replayed on new values (P2P stays opt-in until compared on a multi-GPU RCCL world)
        import lkgd_amd.dist as ld
        from lkgd_amd import replay as _rp
        for allgather in (True, False):
            ld._HALO_ALLGATHER = allgather
            hb2 = torch.zeros(plan.f_local + 2, 3, 5)
            hb2[1:plan.f_local + 1] = local
            with _rp.record() as rec_h:
                exchange_halo(hb2, plan)
            ok = ok and torch.equal(hb2, hb)
            hb2[1:plan.f_local + 1] = 3.0 * local
            rec_h.run()
            want = 3.0 * padded[plan.f0:plan.f0 + plan.f_local + 2]
            ok = ok and torch.equal(hb2, want)
        ld._HALO_ALLGATHER = True
        # pixel re-sharding around the temporal attention (SURVEY.md 8e variant iii): [f_local, HW, C] -> [F, HW/k, C] and back
        from lkgd_amd.dist import frames_to_pixels, pixel_splits, pixels_to_frames
        for HW in (32, 7, 48):
            if HW < world:
                continue
            fullp = torch.arange(frames * HW * 3, dtype=torch.float32).reshape(frames, HW, 3) * 0.5 - 7.0
            mine = fullp[plan.f0:plan.f0 + plan.f_local].clone()
            px = pixel_splits(HW, world)
            ok = ok and sum(px) == HW and all(p > 0 for p in px)
            p0 = sum(px[:plan.shard_index])
            with _rp.record() as rec_p:
                xp = frames_to_pixels(mine, plan)
                back = pixels_to_frames(xp, plan, HW)
            ok = ok and torch.equal(xp, fullp[:, p0:p0 + px[plan.shard_index]])
            ok = ok and torch.equal(back, mine)
            mine.mul_(-2.0)                      # replay on new values in the same buffers
            rec_p.run()
            ok = ok and torch.equal(xp, -2.0 * fullp[:, p0:p0 + px[plan.shard_index]]) and torch.equal(back, mine)
        ok = ok and pixel_splits(9216, 4) == (2304, 2304, 2304, 2304) and pixel_splits(144, 4) == (48, 32, 32, 32)
        # recorded exchange steps (lkgd_amd/replay.py): new values in the same buffers, same plan
        from lkgd_amd import replay
        src = local.clone()
        sums2 = torch.full((1, 32, 2), float(rank + 1))
        with replay.record() as rec:
            got2 = gather_frames(src, plan)
            allreduce_sums(sums2, plan)
        ok = ok and torch.equal(got2, full)
        src.mul_(2.0)
        sums2.fill_(float(10 * (rank + 1)))
        rec.run()
        ok = ok and torch.equal(got2, full * 2.0)
        ok = ok and torch.equal(sums2, torch.full((1, 32, 2), float(10 * sum(range(1, world + 1)))))
        # several batch entries per rank (round 5: both clips of the [start, end] pair on every rank of a CFG half): the exchanges
        # run entry by entry on the (entry, frame, pixel) row layout of the token matrices
        from lkgd_amd.dist_run import ShardInfo
        sh = ShardInfo(plan, None, entries=2)
        ok = ok and sh.B_total == 2 and sh.b0 == 0
        HW, C = 6, 3
        if HW >= world:
            both = torch.arange(2 * frames * HW * C, dtype=torch.float32).reshape(2, frames, HW, C)
            mine2 = both[:, plan.f0:plan.f0 + plan.f_local].reshape(-1, C).contiguous()
            full2 = sh.gather(mine2)
            ok = ok and torch.equal(full2, both.reshape(-1, C))
            px = pixel_splits(HW, world)
            p0 = sum(px[:plan.shard_index])
            xp2 = sh.to_pixels(mine2, HW)
            ok = ok and torch.equal(xp2, both[:, :, p0:p0 + px[plan.shard_index]].reshape(-1, C))
            ok = ok and torch.equal(sh.to_frames(xp2, HW), mine2)
            hb3 = torch.zeros(2, plan.f_local + 2, HW, C)
            hb3[:, 1:plan.f_local + 1] = both[:, plan.f0:plan.f0 + plan.f_local]
            sh.halo(hb3.reshape(-1, C))
            pad2 = torch.cat([torch.zeros(2, 1, HW, C), both, torch.zeros(2, 1, HW, C)], dim=1)
            ok = ok and torch.equal(hb3, pad2[:, plan.f0:plan.f0 + plan.f_local + 2])
        # temporal GroupNorm + Conv3d halo in ONE collective: raw boundary frames and the partial sums in the same all-gather
        from lkgd_amd.dist import SUMS_SLOT, gather_boundary_frames_and_sums
        HWc, Cc = 4, 8
        xb = (torch.arange(2 * frames * HWc * Cc, dtype=torch.float32).reshape(2, frames, HWc, Cc) * 0.25 - 3.0).half()
        mine3 = xb[:, plan.f0:plan.f0 + plan.f_local].contiguous()
        sm = torch.arange(2 * 64, dtype=torch.float32).reshape(2, 32, 2) * (rank + 1) + 0.125
        got = gather_boundary_frames_and_sums([mine3[b, 0] for b in range(2)], [mine3[b, -1] for b in range(2)], sm, plan)
        n = HWc * Cc
        ok = ok and tuple(got.shape) == (world, 2, 2 * n + SUMS_SLOT)
        for r in range(world):
            pr = make_plan(world, r, frames, cfg=False)
            for b in range(2):
                ok = ok and torch.equal(got[r, b, :n], xb[b, pr.f0].reshape(-1))
                ok = ok and torch.equal(got[r, b, n:2 * n], xb[b, pr.f0 + pr.f_local - 1].reshape(-1))
                want = torch.arange(2 * 64, dtype=torch.float32).reshape(2, 64)[b] * (r + 1) + 0.125
                ok = ok and torch.equal(got[r, b, 2 * n:].view(torch.float32), want)     # fp32 bits survive the fp16 carrier
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("frames", [4, 5, 14, 3])
def test_uneven_frame_gather_world2(frames):
    res = sorted(run_world(_worker, 2, frames))
    assert res == [(0, True), (1, True)]


def test_frame_exchanges_world4():
    """14 frames over 4 shards (4, 4, 3, 3): interior ranks have a neighbour on both sides of the Conv3d halo"""
    res = sorted(run_world(_worker, 4, 14))
    assert res == [(r, True) for r in range(4)]


def test_thread_world_collectives_match_their_definitions():
    """tests/thread_world.py (the in-process stand-in for torch.distributed the eight-rank GPU test runs on): sub-groups,
    all-gather, all-to-all with uneven rows, all-reduce"""
    from thread_world import ThreadWorld, run_ranks
    W = 8
    tw = ThreadWorld(W)
    rows = [1, 2, 3, 1]                                   # rows every rank of a group sends to peer 0..3

    def fn(r):
        groups = [tw.new_group([0, 1, 2, 3]), tw.new_group([4, 5, 6, 7])]
        g, si = groups[r // 4], r % 4
        t = torch.full((2,), float(r))
        tw.all_reduce(t, group=g)
        buf = torch.empty(4 * 2)
        tw.all_gather_into_tensor(buf, torch.full((2,), float(r)), group=g)
        inp = torch.arange(7 * 2, dtype=torch.float32).reshape(7, 2) + 100 * r
        out = torch.empty(4 * rows[si], 2)
        tw.all_to_all_single(out, inp, [rows[si]] * 4, rows, group=g)
        tw.barrier()
        return t, buf, out

    res = run_ranks(tw, fn)
    for r, (t, buf, out) in enumerate(res):
        base = 4 * (r // 4)
        assert t.tolist() == [float(sum(range(base, base + 4)))] * 2
        assert buf.tolist() == [float(base + i) for i in range(4) for _ in range(2)]
        si, start = r % 4, sum(rows[:r % 4])
        want = torch.cat([(torch.arange(14, dtype=torch.float32).reshape(7, 2) + 100 * (base + p))[start:start + rows[si]]
                          for p in range(4)])
        assert torch.equal(out, want)


@pytest.mark.parametrize("per_frame", [6 * 4, 16 * 2 * 3], ids=["HWx4", "CxHxW"])
@pytest.mark.parametrize("entries", [1, 2])
@pytest.mark.parametrize("world,cfg,frames", [(2, True, 3),       # CFG halves only: frame_shards == 1
                                              (4, True, 5),       # CFG x (3, 2): the shorter slice travels padded
                                              (4, False, 6),      # cfg_groups == 1 with shards (2, 2, 1, 1)
                                              (8, True, 14)])     # CFG x (4, 4, 3, 3)
def test_noise_gather_and_frame_groups(world, cfg, frames, entries, per_frame, monkeypatch):
    """the once-per-step exchange of both sharded loops (SVD: ``b_local`` entries of HW * 4; DiT: one entry of C * H * W): every
    rank's slice in, the whole tensor out on every rank.  Values encode (entry, frame, element).  And the group builder hands
    every rank the group of its CFG half's frame slices."""
    import lkgd_amd.dist as ld
    from thread_world import ThreadWorld, run_ranks
    tw = ThreadWorld(world)
    monkeypatch.setattr(ld, "dist", tw)
    total = (2 if cfg else 1) * entries
    e, f, k = torch.meshgrid(torch.arange(total), torch.arange(frames), torch.arange(per_frame), indexing="ij")
    full = (10000 * e + 100 * f + k).float()                       # [total, frames, per_frame], exact in fp32

    def fn(r):
        plan = make_plan(world, r, frames, cfg)
        group = ld.new_frame_group(plan)
        gather = ld.NoiseGather(plan, entries, per_frame, torch.float32, "cpu")
        e0 = plan.cfg_index * entries
        got = []
        for scale in (1.0, -2.0):                                  # a second step through the same buffers
            local = scale * full[e0:e0 + entries, plan.f0:plan.f0 + plan.f_local].clone()
            got.append(gather(local).clone())
        return plan, group, got

    for plan, group, got in run_ranks(tw, fn):
        assert got[0].shape == (total, frames * per_frame)
        assert torch.equal(got[0], full.reshape(total, -1)) and torch.equal(got[1], -2.0 * full.reshape(total, -1))
        if plan.frame_shards == 1:
            assert group is None
        else:
            assert group.ranks == plan.frame_group_ranks()


@pytest.mark.parametrize("world,windows", [(2, [(0, 0, 3), (1, 0, 3)]),                               # the CFG halves, whole clip
                                           (4, [(0, 0, 2), (0, 2, 1), (1, 0, 2), (1, 2, 1)])])        # CFG halves x frames (2, 1)
def test_dit_rank_placement_windows_and_row_gather(world, windows, monkeypatch):
    """what a rank of ``DistDiTDenoiser`` answers ``cogvideox.denoise`` for 3 latent frames: (CFG half, first frame, frames) per rank
    written out, against ``make_plan``; the text rows of its half; the shard only where frames are split.  And the noise gather in
    row format: each rank hands in its [f_local h w, C p p] token rows, every rank gets the [cfg F h w, C p p] rows of the whole
    clip (values encode (entry, token, column))"""
    import lkgd_amd.dist as ld
    import lkgd_amd.dist_run as dr
    from thread_world import ThreadWorld, run_ranks
    tw = ThreadWorld(world)
    monkeypatch.setattr(ld, "dist", tw)
    F, C, H, W, p = 3, 16, 8, 12, 2
    hw, width = (H // p) * (W // p), C * p * p
    e, t, k = torch.meshgrid(torch.arange(2), torch.arange(F * hw), torch.arange(width), indexing="ij")
    full = (100000 * e + 100 * t + k).float().reshape(2 * F * hw, width)          # exact in fp32
    lat = torch.arange(F * 5, dtype=torch.float32).reshape(1, F, 5)
    text = torch.arange(2 * 4, dtype=torch.float32).reshape(2, 4)
    shard = object()

    def fn(r):
        plan = make_plan(world, r, F, True)
        place = dr._DiTRankPlacement(plan, shard, C * H * W, "cpu")
        place.gather = ld.NoiseGather(plan, 1, C * H * W, torch.float32, "cpu")       # the values above need fp32
        ci, f0, fl = windows[r]
        assert (plan.cfg_index, plan.f0, plan.f_local) == (ci, f0, fl)
        assert torch.equal(place.frames(lat), lat[:, f0:f0 + fl]) and place.frames(lat).is_contiguous() and place.frames(None) is None
        assert torch.equal(place.text(text), text[ci:ci + 1])
        assert place.shard is (shard if world == 4 else None)
        local = full[(ci * F + f0) * hw:(ci * F + f0 + fl) * hw]
        return [place.noise(scale * local).clone() for scale in (1.0, -2.0)]         # a second step through the same buffers

    for got in run_ranks(tw, fn):
        assert got[0].shape == full.shape and torch.equal(got[0], full) and torch.equal(got[1], -2.0 * full)


def _worker_replay_entries(rank, world, port, frames, q):
    """with several batch entries per rank the joined result of the per-entry exchanges must be refreshed by
    the recorded steps themselves - record, change the inputs in place, replay, compare"""
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from lkgd_amd import replay
        from lkgd_amd.dist import pixel_splits
        from lkgd_amd.dist_run import ShardInfo
        plan = make_plan(world, rank, frames, cfg=False)
        ok = True
        for entries in (1, 2, 3):
            sh = ShardInfo(plan, None, entries=entries)
            HW, C = 8, 3
            both = torch.arange(entries * frames * HW * C, dtype=torch.float32).reshape(entries, frames, HW, C) + 1.0
            mine = both[:, plan.f0:plan.f0 + plan.f_local].reshape(-1, C).clone()
            px = pixel_splits(HW, world)
            p0 = sum(px[:plan.shard_index])
            with replay.record() as rec:
                full = sh.gather(mine)
                xp = sh.to_pixels(mine, HW)
                back = sh.to_frames(xp, HW)
            for scale in (1.0, -3.0, 0.5):
                if scale != 1.0:
                    mine.copy_(scale * both[:, plan.f0:plan.f0 + plan.f_local].reshape(-1, C))
                    rec.run()
                ok = ok and torch.equal(full, scale * both.reshape(-1, C))
                ok = ok and torch.equal(xp, scale * both[:, :, p0:p0 + px[plan.shard_index]].reshape(-1, C))
                ok = ok and torch.equal(back, mine)
            rec.release()
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


def _worker_mirror(rank, world, port, frames, q):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from lkgd_amd import replay
        from lkgd_amd.dist import exchange_with_mirror
        plan = make_plan(world, rank, frames, cfg=False, symmetric=True)
        mp_ = make_plan(world, world - 1 - rank, frames, cfg=False, symmetric=True)
        ok = plan.f_local == mp_.f_local
        HW, W = 3, 4
        full = torch.arange(frames * HW * W, dtype=torch.float32).reshape(frames, HW, W) + 1.0
        mine = full[plan.f0:plan.f0 + plan.f_local].reshape(-1, W).clone()
        with replay.record() as rec:
            got = exchange_with_mirror(mine, plan)
        for scale in (1.0, -2.0):
            if scale != 1.0:
                mine.copy_(scale * full[plan.f0:plan.f0 + plan.f_local].reshape(-1, W))
                rec.run()
            ok = ok and torch.equal(got, scale * full[mp_.f0:mp_.f0 + mp_.f_local].reshape(-1, W))
            # local frame t of the mirror shard is global frame F-1-(f0 + f_local-1-t): the flip of patch/patch.py:471-475
            t = 0
            ok = ok and torch.equal(got.reshape(plan.f_local, HW, W)[plan.f_local - 1 - t], scale * full[frames - 1 - (plan.f0 + t)])
        bad = make_plan(world, rank, frames, cfg=False)            # (3, 3, 2, 2)-style slices are not mirror images of each other
        if bad.splits != plan.splits:
            try:
                exchange_with_mirror(mine, bad)
                ok = False
            except ValueError:
                pass
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,frames", [(4, 6), (3, 7), (2, 6)])
def test_mirror_exchange_of_symmetric_slices(world, frames):
    res = sorted(run_world(_worker_mirror, world, frames))
    assert res == [(r, True) for r in range(world)]


@pytest.mark.parametrize("world,frames", [(2, 5), (4, 6)])
def test_recorded_multi_entry_exchanges_follow_their_inputs(world, frames):
    res = sorted(run_world(_worker_replay_entries, world, frames))
    assert res == [(r, True) for r in range(world)]

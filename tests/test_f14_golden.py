"""All 14 frames of a clip at the REAL width against the reference's own pipeline `__call__` (round 3).

tests/golden/loop_f14_cfg.safetensors <- pipeline/pipeline_stable_video_diffusion_trans.py:545-640 run in fp32 on the CPU of
the build container (tests/golden/make_goldens.py::gen_loop_f14): the real-width stock UNet on 14 frames x 32 x 64 latent
(256 x 512 px, S = 2048), CFG 1 -> 3, 2 Euler steps, every step's latents stored.  This is the fixture that sees the
14-frame temporal attention, the F = 14 Conv3d chain and the temporal GroupNorm across 14 frames end to end - the
full-resolution fixtures carry 2 frames - and the one the frame-sharded run is checked against: CFG-parallel x (7, 7) frame
slices, four ranks sharing the GPU over gloo, each compared with the REFERENCE (not with the single-process HIP loop).
(The reference loop has no guidance-free branch - `noise_pred` is only assigned under classifier-free guidance, :583-595 -
so a 4-way frame split without CFG-parallel, (4,4,3,3), has no reference run to compare with; it stays pinned against the
single-process loop in test_dist_gpu.py.)  Gate: relative L2 <= 2e-2 per step (fp16 loop vs fp32 loop)."""
import os

import pytest
import torch
from safetensors.torch import load_file

pytestmark = pytest.mark.gpu
C1_SEED = 31


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return load_file(os.path.join(golden_dir, "loop_f14_cfg.safetensors"))


def test_hip_loop_14_frames_vs_reference_golden(golden, c1_oracle_model, c1_hip_model):
    from lkgd_amd.pipeline import StableVideoDiffusionPipeline
    g = golden
    ck = float(sum(p.detach().double().abs().sum() for p in c1_oracle_model.parameters()))
    assert abs(ck - g["checksum"].item()) <= 1e-9 * ck, "regenerated weights differ from the ones the reference ran with"
    pipe = StableVideoDiffusionPipeline(unet=c1_hip_model)
    steps = []
    out = pipe(None, height=256, width=512, num_frames=14, num_inference_steps=2, latents=g["latents0"], output_type="latent",
               image_embeddings=g["image_embeddings"], image_latents=g["image_latents"].half(), fps=7, motion_bucket_id=127,
               noise_aug_strength=0.02,
               callback_on_step_end=lambda p, i, t, kw: (steps.append(kw["latents"].clone()), {})[1])
    assert out.frames.shape == g["final"].shape and torch.isfinite(out.frames.float()).all()
    for i, st in enumerate(steps):
        assert _rel(st, g["step_latents"][i]) < 2e-2, i
    rel = _rel(out.frames, g["final"])
    print(f"\n14-frame loop vs reference: final rel L2 {rel:.3e}")
    assert rel < 2e-2


def _worker(rank, world, port, gpath, wpath, q):
    import time
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.set_num_threads(max(1, int(os.environ.get("LKGD_TEST_HOST_CPUS", os.cpu_count() or 8)) // world))   # the ranks share the box's host cores
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from lkgd_amd import unet as pu
        from lkgd_amd.dist_run import DistDenoiser
        from lkgd_amd.pipeline import StableVideoDiffusionPipeline
        t0 = time.time()
        g = load_file(gpath)
        with torch.device("meta"):
            m = pu.UNetSpatioTemporalConditionControlNetModel(pu.UNetConfig())
        m = m.to(torch.float16).to_empty(device="cpu")
        m.load_state_dict(torch.load(wpath, map_location="cpu", mmap=True, weights_only=True), strict=True)
        dev = torch.device("cuda", 0)
        pipe = StableVideoDiffusionPipeline(unet=m.to(dev))
        print(f"[rank {rank}] model on the GPU after {time.time() - t0:.0f} s", flush=True)
        pipe.scheduler.set_timesteps(2)
        runner = DistDenoiser(pipe, world, rank, 14, cfg=True)
        ids = torch.tensor([[6.0, 127.0, 0.02]] * 2)
        # `latents0` of the fixture is what the reference was handed; it scales by init_noise_sigma itself (:519)
        lat = (g["latents0"] * float(pipe.scheduler.init_noise_sigma)).half().to(dev)
        out = runner.denoise(lat, g["image_latents"].half().to(dev), g["image_embeddings"].half().to(dev), ids.to(dev), 2, 1.0, 3.0)
        print(f"[rank {rank}] 2 Euler steps done after {time.time() - t0:.0f} s", flush=True)
        q.put({"rank": rank, "out": out.float().cpu().numpy()})
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [4, 2])
def test_sharded_cfg_x_7_7_loop_vs_reference_golden(golden, golden_dir, c1_hip_model, world):
    """4 ranks = CFG-parallel x frame slices (7, 7) of the 14 frames (the 4-GPU layout of DESIGN.md section 6): the temporal
    attention's all-to-all re-sharding, Conv3d halos, all-reduced temporal GroupNorm sums - every rank's result against the
    REFERENCE's fp32 run.  2 ranks = CFG-parallel only (the 2-GPU layout): every rank runs ONE batch entry with all 14 frames -
    the one-launch temporal attention and the fused feed-forwards with the second entry's context-table offset.  The eight-rank
    CFG x (4,4,3,3) layout runs in tests/test_zz_eight_ranks_gpu.py as threads (this pool admits six GPU processes per card, pytest included)."""
    from dist_support import run_world
    gpath = os.path.join(golden_dir, "loop_f14_cfg.safetensors")
    # the ranks load the session model's fp16 weights from shared memory (3 GB) instead of re-drawing 1.5 B parameters each
    wpath = "/dev/shm/lkgd_f14_weights_%d.pt" % os.getpid()
    torch.save({k: v.detach().cpu() for k, v in c1_hip_model.state_dict().items()}, wpath)
    try:
        results = run_world(_worker, world, gpath, wpath, timeout=900, join=120)
    finally:
        os.remove(wpath)
    for r in results:
        rel = _rel(r["out"], golden["final"])
        assert rel < 2e-2, f"rank {r['rank']} of {world}: sharded 14-frame loop vs the reference: relative L2 {rel:.3e}"

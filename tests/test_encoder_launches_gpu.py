"""The launch list of one forward of the two pre-LN image encoders (lkgd_amd/vit.py, lkgd_amd/clip.py over lkgd_amd/encoder.py): the
C-ABI entry points in order, written out as prologue + per-layer block x layers + tail.  The lists were recorded on the commit before
the two forwards were folded into one layer loop; the kernels' values are pinned elsewhere (test_vit.py, test_clip_gpu.py).  The three
cases cover both attention kernels, a head width that is not 64, both activations, and more than one image in the per-image embedding
loop."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

LN, GEMM = "lkgd_layernorm", "lkgd_gemm_f16"


def _expected(images, layers, attn, quick_gelu=False, patchify=False, pre_norm=False):
    prologue = (["lkgd_vit_patchify"] if patchify else []) + [GEMM] * images + ([LN] if pre_norm else [])
    #        LN, q|k|v, attention, out-projection + residual, LN, fc1 (GELU in the epilogue, or + silu), fc2 + residual
    block = [LN, GEMM, attn, GEMM, LN, GEMM] + (["lkgd_silu"] if quick_gelu else []) + [GEMM]
    tail = [LN, GEMM]                    # the class rows: norm, then head / projection
    return prologue + block * layers + tail


def _recorded(run):
    """one eager warm-up, then a recorded call: the entry-point names, in order"""
    from lkgd_amd import replay
    run()
    torch.cuda.synchronize()
    with replay.strict(False):                 # only the launch list is of interest here: nothing is replayed
        with replay.record() as p:
            run()
    torch.cuda.synchronize()
    names = [name for _, _, name, _ in p.calls]
    p.release()
    return names


def _check(got, want):
    first = next((k for k, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, (len(got), len(want), first, got[first:first + 6], want[first:first + 6])


def test_vit_tiny_launch_list():
    """TINY_VIT (2 blocks, 2 heads of 64) on three 40x56 images, the input of test_vit_tiny_vs_oracle"""
    from lkgd_amd import vit as pv
    from oracle import vit as ov
    m = pv.VisionTransformer(pv.ViTConfig(**ov.TINY_VIT.__dict__)).half().to(DEV)
    x = torch.rand(3, 3, 40, 56, generator=torch.Generator().manual_seed(6)).to(DEV)
    got = _recorded(lambda: m(x))
    assert len(m._pk.layers) == 2
    _check(got, _expected(3, 2, "lkgd_attn_spatial", patchify=True))


@pytest.mark.parametrize("act", ["gelu", "quick_gelu"])
def test_clip_small_launch_list(act):
    """the small CLIP of test_clip_small_matches_transformers: 640 wide, 2 layers, 8 heads of 80, 17 tokens, two images"""
    from lkgd_amd.clip import CLIPVisionConfig, CLIPVisionModelWithProjection
    cfg = CLIPVisionConfig(hidden_size=640, intermediate_size=2560, num_hidden_layers=2, num_attention_heads=8, patch_size=14,
                           image_size=56, projection_dim=512, hidden_act=act)
    torch.manual_seed(3)
    m = CLIPVisionModelWithProjection(cfg).to(DEV).half()
    torch.manual_seed(5)
    x = torch.randn(2, 3, 56, 56).to(DEV)
    got = _recorded(lambda: m(x))
    assert m._pk.layers[0].act == act
    _check(got, _expected(2, 2, "lkgd_attn_dense", quick_gelu=act == "quick_gelu", pre_norm=True))

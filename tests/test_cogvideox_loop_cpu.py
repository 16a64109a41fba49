"""Host side of the CogVideoX loop kernels without a GPU: the three entry points refuse bad arguments with the documented codes before any
launch; ``pack_lk_tokens`` packs the 18 operands of the DiT's latent-knowledge fuse; ``fused_text`` has no CPU path; nothing under
lkgd_amd/ calls rocFFT or ATen's interpolation any more."""
import ctypes as C
import glob
import os

import pytest
import torch

from c_interface import ALIGN, NULL, SHAPE, Host, entry
from cogvideox_support import REPO, tiny_cpu_model

def test_lk_fuse_tokens_refusals():
    h = Host()
    call = entry("lkgd_lk_fuse_tokens", e=h.p, lde=4096, d=h.p, f=h.p, B=2, L=5, Bd=1, w=h.w, out=h.p, ldo=4096)
    for k in ("e", "d", "f", "w", "out"):
        assert call(**{k: None}) == NULL, k
    for i in (0, 7, 17):
        w = (C.c_void_p * 18)(*[h.p] * 18)
        w[i] = None
        assert call(w=w) == NULL, i
    for kw in (dict(B=0), dict(B=-1), dict(L=0), dict(Bd=0), dict(Bd=3), dict(B=3, Bd=2), dict(lde=4092), dict(ldo=4088),
               dict(B=1 << 20, L=1 << 20)):
        assert call(**kw) == SHAPE, kw
    w = (C.c_void_p * 18)(*[h.p] * 18)
    w[16] = h.p + 4
    for kw in (dict(e=h.p + 4), dict(out=h.p + 2), dict(lde=4098), dict(ldo=4100), dict(w=w)):
        assert call(**kw) == ALIGN, kw
    assert call(Bd=2, B=2, lde=4100, ldo=4104, e=None) == NULL            # NULL comes first


def test_dit_glue_refusals():
    h = Host()
    patch = entry("lkgd_dit_patch_rows", latents=h.p, latents_is_f32=0, image_latents=h.p, B=1, F=3, C=16, H=8, W=12, p=2, rows_out=h.p,
                  ldp=128)
    step = entry("lkgd_dit_cfg_ddim_step", noise_rows=h.p, ldn=64, latents=h.p, latents_is_f32=1, B=1, F=3, C=16, H=8, W=12, p=2, cfg=2,
                 guidance=3.0, a=0.9, b=0.1, sqrt_alpha=0.8, sqrt_beta=0.6)
    assert patch(latents=None) == NULL and patch(rows_out=None) == NULL
    assert step(noise_rows=None) == NULL and step(latents=None) == NULL
    for name, fn, ld in (("patch", patch, "ldp"), ("step", step, "ldn")):
        for kw in (dict(p=1), dict(p=4), dict(W=13), dict(H=7), dict(B=0), dict(F=0), dict(C=0), dict(C=3), {ld: 56},
                   {ld: 132}):                         # p = 1, odd W, odd H, empty, C * 4 % 8, short ld, ld % 8
            assert fn(**kw) == SHAPE, (name, kw)
    assert patch(ldp=64) == SHAPE                      # 2C channels with image latents: 128 columns
    assert patch(image_latents=None, ldp=56) == SHAPE  # C channels without them: 64
    assert step(cfg=0) == SHAPE and step(cfg=3) == SHAPE
    assert patch(rows_out=h.p + 8) == ALIGN and step(noise_rows=h.p + 2) == ALIGN


def test_pack_lk_tokens_shapes_and_hamilton():
    from lkgd_amd import lk_fuse
    m = tiny_cpu_model(4242)
    ws, ptrs = lk_fuse.pack_lk_tokens(m)
    assert [tuple(w.shape) for w in ws] == lk_fuse.LK_TOKENS_SHAPES == [
        (256, 16), (256, 4), (256, 4), (256,), (1024, 512), (512,), (129,), (129,), (512, 256), (256,), (512, 256), (256,), (5,), (5,),
        (1024, 512), (512,), (512, 4096), (4096,)]
    assert all(w.dtype == torch.float32 and w.is_contiguous() for w in ws)
    assert len(ptrs) == 18 and [int(x) for x in ptrs] == [w.data_ptr() for w in ws]
    # Hamilton blocks: block (row a, column b) of the (in, out) matrix is sign * component (core_qnn quaternion_linear)
    table = [[(1, "r"), (1, "i"), (1, "j"), (1, "k")], [(-1, "i"), (1, "r"), (1, "k"), (-1, "j")],
             [(-1, "j"), (-1, "k"), (1, "r"), (1, "i")], [(-1, "k"), (1, "j"), (-1, "i"), (1, "r")]]
    for idx, q in ((4, m.quaternion_lora_fuse), (8, m.quaternion_lora_fuse_fft_mag), (10, m.quaternion_lora_fuse_fft_pha)):
        comp = dict(r=q.r_weight, i=q.i_weight, j=q.j_weight, k=q.k_weight)
        n, o = q.r_weight.shape
        for a in range(4):
            for b in range(4):
                sign, c = table[a][b]
                assert torch.equal(ws[idx][a * n:(a + 1) * n, b * o:(b + 1) * o], sign * comp[c].detach().float()), (idx, a, b)
        assert torch.equal(ws[idx + 1], q.bias.detach().float())
    # the plain operands
    assert torch.equal(ws[0], m.quaternion_lora_lconv.weight.detach().reshape(256, 16))
    assert torch.equal(ws[16], m.quaternion_lora_fuse_sf[2].weight.detach().T) and torch.equal(ws[14], m.quaternion_lora_fuse_sf[0].weight.detach().T)
    assert torch.equal(ws[12][:4], m.quaternion_lora_fuse_fft_mag0.weight.detach().reshape(4)) \
        and torch.equal(ws[12][4:], m.quaternion_lora_fuse_fft_mag0.bias.detach())
    assert torch.equal(ws[3], m.quaternion_lora_texts.detach()) and torch.equal(ws[7], m.quaternion_lora_texts_fft_pha.detach())


def test_fused_text_on_a_cpu_model_raises():
    from lkgd_amd._lib import LkgdHipError
    m = tiny_cpu_model(4242)
    with pytest.raises(LkgdHipError, match="no CPU path"):
        m.fused_text(torch.zeros(1, 4, 4096), torch.zeros(1, 1, 1000), torch.zeros(1, 1, 1000))


def test_package_source_has_no_fft_and_no_interpolate():
    """LKGD's own math in the DiT path depends on no rocFFT / ATen kernel choice: the words occur nowhere under lkgd_amd/"""
    files = glob.glob(os.path.join(REPO, "lkgd_amd", "**", "*.py"), recursive=True)
    assert len(files) > 10
    for path in files:
        src = open(path).read()
        assert "torch.fft" not in src and "F.interpolate" not in src, path
    src = open(os.path.join(REPO, "lkgd_amd", "cogvideox.py")).read()
    assert "lkgd_lk_fuse_tokens" in src and "dit_patch_rows" in src and "dit_cfg_ddim_step" in src and "def forward_rows" in src

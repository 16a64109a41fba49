"""The rotary CogVideoX DiT (CogVideoX-5B-I2V) on the MI355X: ``lkgd_qk_norm_rope`` (include/lkgd_hip_dit.h) bit for bit against
``lkgd_layernorm`` + the reference's rotation in torch fp32, its footprint cases (tests/footprint.py) and refusals; LayerNorm
rows of 2056 .. 3072 channels; the HIP forward against tests/golden/cogvideox_rope.safetensors (the reference's own in-tree
forward, make_goldens_cogvideox_rope.py), the 3072-wide model and the DDIM loop against the fp32 twin
(tests/cogvideox_rope_oracle.py), and the loop over two ranks against one process."""
import os

import pytest
import torch
import torch.nn.functional as F
from safetensors.torch import load_file

import cogvideox_rope_oracle as ro
from cogvideox_support import DEV, DIT_SEED, dit_inputs as _inputs, hip_twin, loop_inputs, rel as _rel
from c_interface import ALIGN, NULL, SHAPE, entry
from footprint import run_case

gpu = pytest.mark.gpu

#: every name in lkgd_amd._lib.DIT_SYMBOLS -> its footprint tests in this module (the rule REGISTRY keeps for _lib.SYMBOLS in
#: tests/test_footprint_gpu.py)
FOOTPRINT = {
    "lkgd_qk_norm_rope": ["test_qk_norm_rope_footprint"],
}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return load_file(os.path.join(golden_dir, "cogvideox_rope.safetensors"))


@pytest.fixture(scope="module")
def tiny():
    """(twin, HIP model) of the fixture's tiny rotary DiT; neither is modified by a test"""
    o = ro.seeded_model(ro.TINY_ROPE_DIT, DIT_SEED)
    return o, hip_twin(o, ro.TINY_ROPE_DIT, DEV)


# --------------------------------------------------------------------------------------------------------------- the kernel
def _qk_case(heads, rpb, split, seed):
    """2 batch entries; q and k with a per-head offset and scale so that the statistics differ from head to head; tables of
    unit-modulus (cos, sin) pairs whose two entries of a pair DIFFER (the kernel must read cos[2i] and cos[2i+1] where the
    formula says so - real tables repeat them)"""
    g = torch.Generator().manual_seed(seed)
    rows = 2 * rpb
    q = (torch.randn(rows, heads, 64, generator=g) * (1 + torch.arange(heads)[None, :, None] % 5) + torch.randn(1, heads, 1, generator=g))
    k = torch.randn(rows, heads, 64, generator=g) * 3 - 1
    v = [1 + 0.3 * torch.randn(64, generator=g) if i % 2 == 0 else 0.3 * torch.randn(64, generator=g) for i in range(4)]
    ang = torch.rand(rpb - split, 64, generator=g) * 6.283
    return (q.reshape(rows, heads * 64).half(), k.reshape(rows, heads * 64).half(), [t.float() for t in v], ang.cos().float(),
            ang.sin().float())


def _composed(x, heads, gamma, beta, eps, cos, sin, rpb, split):
    """what the kernel fuses, unfused: lkgd_layernorm on the [rows * heads, 64] view (on the GPU), then - video rows only - the
    reference's apply_rotary_emb in torch fp32 ops on the fp16-rounded norm, then .half()"""
    from lkgd_amd import ops
    rows = x.shape[0]
    n = ops.layernorm(x.reshape(rows * heads, 64).contiguous(), gamma, beta, eps).view(rows, heads, 64)
    if cos is None or split == rpb:
        return n.reshape(rows, heads * 64)
    vid = (torch.arange(rows, device=x.device) % rpb) >= split
    xv = n[vid].view(-1, rpb - split, heads, 64)                        # [B, video rows, heads, 64]
    c, s = cos[None, :, None, :], sin[None, :, None, :]
    x_real, x_imag = xv.reshape(*xv.shape[:-1], -1, 2).unbind(-1)
    x_rot = torch.stack([-x_imag, x_real], dim=-1).flatten(3)
    out = n.clone()
    out[vid] = (xv.float() * c + x_rot.float() * s).half().reshape(-1, heads, 64)
    return out.reshape(rows, heads * 64)


def _window(t, extra=64, col0=8):
    """a column window of a wider buffer (ld > heads * 64) whose surroundings are NaN"""
    buf = torch.full((t.shape[0], t.shape[1] + extra), float("nan"), dtype=t.dtype, device=t.device)
    buf[:, col0:col0 + t.shape[1]] = t
    return buf, buf[:, col0:col0 + t.shape[1]]


@gpu
@pytest.mark.parametrize("heads", [2, 8, 11, 16, 30, 48])
def test_qk_norm_rope_bitwise(heads):
    """a wave walks a token's heads 16 at a time (4 lanes per head): 2 / 8 / 11 heads are a masked tail only, 16 exactly one
    step, 30 (the 2B count) one step and a tail, 48 (5B) three steps.  rows_per_batch 5 and 37 with 2 batch entries: 10 rows =
    3 workgroups of 4 waves with a ragged last one, 74 rows = 19.  split 0 (no text), 2, rows_per_batch (no video row).
    q and k are column windows of wider NaN-filled buffers.  Norm-only mode == lkgd_layernorm, with tables == the composition,
    both bit for bit: the kernel performs lkgd_layernorm's arithmetic for a 64-channel row (4 lanes x 2 vectors, element and
    shuffle order, rsqrtf) and the rotation's two products and one sum are IEEE fp32 operations with contraction off, as torch's
    separate mul / mul / add kernels perform them."""
    from lkgd_amd import ops
    eps = 1e-6
    for rpb in (5, 37):
        for split in (0, 2, rpb):
            q, k, (gq, bq, gk, bk), cos, sin = (_dev(t) for t in _qk_case(heads, rpb, split, 100 * heads + rpb + split))
            tag = (heads, rpb, split)
            for tables in (None, (cos, sin)):
                (qb, qw), (kb, kw) = _window(q), _window(k, extra=24, col0=16)
                ops.qk_norm_rope(qw, kw, heads, (gq, bq), (gk, bk), eps, tables, rpb, split)
                c, s = tables if tables is not None else (None, None)
                rq, rk = _composed(q, heads, gq, bq, eps, c, s, rpb, split), _composed(k, heads, gk, bk, eps, c, s, rpb, split)
                assert torch.equal(qw, rq), (tag, tables is not None, "q", (qw.float() - rq.float()).abs().max().item())
                assert torch.equal(kw, rk), (tag, tables is not None, "k", (kw.float() - rk.float()).abs().max().item())
                for buf, w in ((qb, qw), (kb, kw)):                        # nothing outside the live columns was written
                    assert int(torch.isnan(buf).sum()) == buf.numel() - w.numel()
                if tables is not None and split < rpb:                      # the rotation acts, and only on video rows
                    nq = _composed(q, heads, gq, bq, eps, None, None, rpb, split)
                    vid = (torch.arange(2 * rpb, device=DEV) % rpb) >= split
                    assert torch.equal(qw[~vid], nq[~vid]) and not torch.equal(qw[vid], nq[vid])


def _dev(t):
    return [x.to(DEV) for x in t] if isinstance(t, list) else t.to(DEV)


#: qk_norm_rope_kernel runs at most 4096 workgroups of 4 tokens (one per wave): the smallest token count at which a workgroup runs
#: its loop body three times, plus a ragged rest
QK_LOOP_TOKENS = 3 * 4096 * 4 + 5              # 49 157


@gpu
def test_qk_norm_rope_three_loop_iterations():
    """one batch entry of 49 157 tokens with 226 text rows: the 32-bit ``tok % rows_per_batch`` and the table row ``r - split`` are
    used far from zero, and every workgroup walks its loop three or four times.  The statement of test_qk_norm_rope_bitwise:
    with tables == the composition, norm only == lkgd_layernorm, bit for bit.  Row r of q and k is scaled by 0.05 + r % 97 and
    the table rows all differ, so a token, a table row or a statistic taken from another loop iteration cannot pass"""
    from lkgd_amd import ops
    heads, rpb, split, eps = 2, QK_LOOP_TOKENS, 226, 1e-6
    g = torch.Generator().manual_seed(49157)
    amp = (0.05 + (torch.arange(rpb) % 97).float())[:, None]
    q = ((torch.randn(rpb, heads * 64, generator=g) + 0.3) * amp).half().to(DEV)
    k = ((torch.randn(rpb, heads * 64, generator=g) * 3 - 1) * amp).half().to(DEV)
    gq, bq, gk, bk = (_dev(t) for t in [1 + 0.3 * torch.randn(64, generator=g), 0.3 * torch.randn(64, generator=g),
                                        1 + 0.3 * torch.randn(64, generator=g), 0.3 * torch.randn(64, generator=g)])
    ang = torch.rand(rpb - split, 64, generator=g) * 6.283
    cos, sin = ang.cos().float().to(DEV), ang.sin().float().to(DEV)
    for tables in (None, (cos, sin)):
        (qb, qw), (kb, kw) = _window(q), _window(k, extra=24, col0=16)
        ops.qk_norm_rope(qw, kw, heads, (gq, bq), (gk, bk), eps, tables, rpb, split)
        c, s = tables if tables is not None else (None, None)
        rq, rk = _composed(q, heads, gq, bq, eps, c, s, rpb, split), _composed(k, heads, gk, bk, eps, c, s, rpb, split)
        for name, got, ref in (("q", qw, rq), ("k", kw, rk)):
            bad = torch.nonzero((got != ref).any(dim=1)).flatten()
            assert bad.numel() == 0, (tables is not None, name, bad.numel(), bad[:8].tolist(), (got.float() - ref.float()).abs().max().item())
        for buf, w in ((qb, qw), (kb, kw)):                                # nothing outside the live columns was written
            assert int(torch.isnan(buf).sum()) == buf.numel() - w.numel()
        if tables is not None:                                              # the rotation acts, and only on video rows
            nq = _composed(q, heads, gq, bq, eps, None, None, rpb, split)
            assert torch.equal(qw[:split], nq[:split]) and not torch.equal(qw[split:], nq[split:])
            assert bool((qw[split:] != nq[split:]).any(dim=1).all())        # on every one of them


@gpu
@pytest.mark.parametrize("heads,rpb,split,norm_only", [(2, 5, 2, 0), (11, 37, 2, 0), (48, 5, 0, 0), (30, 37, 37, 0), (8, 37, 2, 1)])
def test_qk_norm_rope_footprint(heads, rpb, split, norm_only):
    """q and k in place between pattern guards and column gaps, the tables and the four affine vectors between NaN guards: the
    kernel writes q's and k's live columns and rows only, NaN next to every operand changes nothing, and the result equals the
    composition and the run on compact copies bit for bit"""
    from test_footprint_gpu import _lib_, _ok, _st, flat_in
    lib = _lib_()
    q, k, aff, cos, sin = _qk_case(heads, rpb, split, 7 * heads + rpb)
    rows, eps = 2 * rpb, 1e-6
    if rpb == split:            # no video row: a one-row table that must never be read (all NaN)
        cos = sin = torch.full((1, 64), float("nan"))

    def case(W):
        qv = W.inout(q, pad=8, col0=8, name="q")
        kv = W.inout(k, pad=24, col0=0, name="k")
        gq, bq, gk, bk = (flat_in(W, t, n) for t, n in zip(aff, ("gamma_q", "beta_q", "gamma_k", "beta_k")))
        cv, sv = (W.inp(t, pad=4, name=n) for t, n in ((cos, "cos"), (sin, "sin")))
        _ok(lib.lkgd_qk_norm_rope(qv.data_ptr(), qv.stride(0), kv.data_ptr(), kv.stride(0), rows, heads, gq.data_ptr(), bq.data_ptr(),
                                  gk.data_ptr(), bk.data_ptr(), eps, None if norm_only else cv.data_ptr(),
                                  None if norm_only else sv.data_ptr(), cv.stride(0), rpb, split, _st()), "qk_norm_rope")
        return {"q": qv, "k": kv}

    def refs():
        gq, bq, gk, bk = _dev(aff)
        c, s = (None, None) if norm_only or rpb == split else (cos.to(DEV), sin.to(DEV))
        return {"q": _composed(q.to(DEV), heads, gq, bq, eps, c, s, rpb, split),
                "k": _composed(k.to(DEV), heads, gk, bk, eps, c, s, rpb, split)}

    def close(got, ref, what):
        assert torch.equal(got, ref), (what, (got.float() - ref.float()).abs().max().item())
    run_case(case, DEV, refs, close, True, sync=torch.cuda.synchronize)


@gpu
def test_qk_norm_rope_refusals():
    """every refusal returns its code and launches nothing: q and k come back untouched"""
    from test_footprint_gpu import _st
    from lkgd_amd import ops
    from lkgd_amd._lib import LkgdHipError
    heads, rpb, split = 3, 5, 2
    q, k, aff, cos, sin = (_dev(t) for t in _qk_case(heads, rpb, split, 1))
    wide = torch.zeros(10, heads * 64 + 4, dtype=torch.float16, device=DEV)          # a row stride that is no multiple of 8
    odd = torch.zeros(10 * heads * 64 + 8, dtype=torch.float16, device=DEV)[1:]      # 2 bytes off a 16-byte boundary
    oddf = torch.zeros(3 * 64 + 8, dtype=torch.float32, device=DEV)[1:]
    q0, k0 = q.clone(), k.clone()
    call = entry("lkgd_qk_norm_rope", q=q.data_ptr(), ldq=heads * 64, k=k.data_ptr(), ldk=heads * 64, rows=10, heads=heads,
                 gamma_q=aff[0].data_ptr(), beta_q=aff[1].data_ptr(), gamma_k=aff[2].data_ptr(), beta_k=aff[3].data_ptr(), eps=1e-6,
                 cos_t=cos.data_ptr(), sin_t=sin.data_ptr(), ldt=64, rows_per_batch=rpb, split=split, stream=_st())
    for kw, rc in ((dict(q=None), NULL), (dict(k=None), NULL), (dict(gamma_q=None), NULL), (dict(beta_k=None), NULL),
                   (dict(cos_t=None), NULL), (dict(sin_t=None), NULL),                      # exactly one table
                   (dict(heads=0), SHAPE), (dict(heads=-1), SHAPE), (dict(rows=0), SHAPE), (dict(rows=9), SHAPE),   # rows % rpb
                   (dict(rows_per_batch=0), SHAPE), (dict(split=-1), SHAPE), (dict(split=rpb + 1), SHAPE),
                   (dict(ldt=56), SHAPE), (dict(ldq=heads * 64 - 8), SHAPE),
                   (dict(q=wide.data_ptr(), ldq=heads * 64 + 4), ALIGN), (dict(k=wide.data_ptr(), ldk=heads * 64 + 4), ALIGN),
                   (dict(q=odd.data_ptr()), ALIGN), (dict(k=odd.data_ptr()), ALIGN),
                   (dict(cos_t=oddf.data_ptr()), ALIGN), (dict(sin_t=oddf.data_ptr()), ALIGN), (dict(ldt=66), ALIGN)):
        assert call(**kw) == rc, (kw, rc)
    torch.cuda.synchronize()
    assert torch.equal(q, q0) and torch.equal(k, k0)
    # the Python side's own errors: dtype, device, shape of the tables
    nq, nk = (aff[0], aff[1]), (aff[2], aff[3])
    for bad in (lambda: ops.qk_norm_rope(q.float(), k, heads, nq, nk, 1e-6, (cos, sin), rpb, split),
                lambda: ops.qk_norm_rope(q.cpu(), k, heads, nq, nk, 1e-6, (cos, sin), rpb, split),
                lambda: ops.qk_norm_rope(q, k, heads, nq, nk, 1e-6, (cos.half(), sin), rpb, split),
                lambda: ops.qk_norm_rope(q, k, heads, nq, nk, 1e-6, (cos[:2], sin[:2]), rpb, split),
                lambda: ops.qk_norm_rope(q, k[:, :64], heads, nq, nk, 1e-6, (cos, sin), rpb, split),
                lambda: ops.qk_norm_rope(q, k, heads, (aff[0][:32], aff[1]), nk, 1e-6, (cos, sin), rpb, split)):
        with pytest.raises(LkgdHipError):
            bad()
    assert torch.equal(q, q0) and torch.equal(k, k0)


# ------------------------------------------------------------------------------------------------- LayerNorm up to 3072 channels
@gpu
@pytest.mark.parametrize("C_", [2056, 3064, 3072])
def test_layernorm_rows_up_to_3072(C_):
    """one row per wave, six 16-byte vectors per lane: 2056 = the first width past the four-vector program (lane 0 alone holds
    a fifth vector), 3064 = one vector short of full, 3072 = the 5B width; 37 rows = ten workgroups with a ragged last one.
    The bounds of test_dit_kernels_vs_torch's wide rows"""
    from lkgd_amd import ops
    g = torch.Generator().manual_seed(C_)
    x = torch.randn(37, C_, generator=g).half().to(DEV)
    ga, be = torch.randn(C_, generator=g).to(DEV), torch.randn(C_, generator=g).to(DEV)
    ea = (ops.layernorm(x, ga, be, 1e-5).float() - F.layer_norm(x.float(), (C_,), ga, be, 1e-5)).abs().max().item()
    ep = (ops.layernorm(x, None, None, 1e-5).float() - F.layer_norm(x.float(), (C_,), eps=1e-5)).abs().max().item()
    print(f"\nLayerNorm C = {C_}: max abs error affine {ea:.2e}, plain {ep:.2e}")
    assert ea < 8e-3 and ep < 4e-3


# ------------------------------------------------------------------------------------------------------------------ the forward
@gpu
def test_hip_rotary_dit_forward_vs_reference_golden(golden, tiny):
    """the bounds of test_hip_dit_forward_vs_reference_golden (the same forward without rotary embeddings); with identity tables
    the same forward must MISS the reference's output: the rotation is not lost in the tolerance"""
    o, m = tiny
    i = {k: v.to(DEV) for k, v in _inputs(ro.TINY_ROPE_DIT).items()}
    cos, sin = golden["cos"], golden["sin"]
    out = m(i["hidden"], i["text"], i["t"], i["domain"], i["flow"], image_rotary_emb=(cos, sin), return_dict=False)[0]
    r, a = _rel(out, golden["out"]), (out.float().cpu() - golden["out"]).abs().max().item()
    print(f"\nHIP rotary CogVideoX DiT forward vs the reference: rel L2 {r:.3e}, max abs {a:.3e}")
    assert out.shape == golden["out"].shape and r < 1e-2 and a < 5e-2
    ident = m(i["hidden"], i["text"], i["t"], i["domain"], i["flow"], image_rotary_emb=(torch.ones_like(cos), torch.zeros_like(sin)),
              return_dict=False)[0]
    miss = _rel(ident, golden["out"])
    print(f"identity tables: rel L2 {miss:.3f} from the reference's output, {_rel(ident, golden['out_no_rope']):.3e} from its own")
    assert miss >= 0.1 and _rel(ident, golden["out_no_rope"]) < 1e-2


@gpu
def test_hip_rotary_dit_refusals(tiny):
    from lkgd_amd import cogvideox as pc
    from lkgd_amd._lib import LkgdHipError
    o, m = tiny
    cfg = ro.TINY_ROPE_DIT
    i = {k: v.to(DEV) for k, v in _inputs(cfg).items()}
    with pytest.raises(LkgdHipError, match="image_rotary_emb"):               # a rotary model needs its tables
        m(i["hidden"], i["text"], i["t"], i["domain"], i["flow"])
    cos, sin = pc.rotary_tables(m.config, 3, 4, 6)
    with pytest.raises(LkgdHipError, match="image_rotary_emb"):               # of the clip's size
        m(i["hidden"], i["text"], i["t"], i["domain"], i["flow"], image_rotary_emb=(cos[:-1], sin[:-1]))
    with pytest.raises(ValueError, match="learned"):                          # the learned table has rows for the configured grid only
        c2, s2 = pc.rotary_tables(m.config, 2, 4, 6)
        m(i["hidden"][:, :2], i["text"], i["t"], i["domain"], i["flow"], image_rotary_emb=(c2, s2))


@gpu
def test_hip_rotary_dit_real_width_vs_twin():
    """the 5B model's width (48 heads x 64 = 3072 channels: the six-vector LayerNorm rows, 3072 / 12 288-column GEMMs, three
    full head steps of lkgd_qk_norm_rope, the learned table in both embedding GEMMs, all 226 text tokens) with 2 layers on a
    small video (5 latent frames of 16 x 24 -> 480 video tokens), against the twin"""
    from lkgd_amd import cogvideox as pc
    cfg = ro.RopeDiTConfig(num_attention_heads=48, in_channels=32, num_layers=2, sample_width=24, sample_height=16, sample_frames=17)
    o = ro.seeded_model(cfg, DIT_SEED)
    m = hip_twin(o, cfg, DEV)
    i = _inputs(cfg, seed=7)
    cos, sin = pc.rotary_tables(m.config, 5, 8, 12)
    with torch.no_grad():
        ref = o(i["hidden"], i["text"], i["t"], i["domain"], i["flow"], image_rotary_emb=ro.rotary_tables(cfg, 5, 8, 12))[0]
    out = m(i["hidden"].to(DEV), i["text"].to(DEV), i["t"].to(DEV), i["domain"].to(DEV), i["flow"].to(DEV),
            image_rotary_emb=(cos, sin), return_dict=False)[0]
    r = _rel(out, ref)
    print(f"\nreal-width (3072) 2-layer rotary DiT vs twin: rel L2 {r:.3e}")
    assert out.shape == ref.shape == (2, 5, 16, 16, 24) and r < 1e-2


@gpu
def test_hip_rotary_dit_loop_vs_twin(tiny):
    """pipeline_cogvideox_image2video.py:819-885: 4 DDIM steps with dynamic CFG, tiny rotary DiT, ``denoise`` building its own
    tables, against the twin's loop; the bounds of test_hip_dit_loop_vs_oracle"""
    from lkgd_amd import cogvideox as pc
    from oracle import cogvideox as oc
    cfg = ro.TINY_ROPE_DIT
    o, m = tiny
    lat, img, pe, dom, flow = loop_inputs(cfg)
    rope = ro.rotary_tables(cfg, 3, cfg.sample_height // 2, cfg.sample_width // 2)
    ref_steps, got_steps = [], []
    ref = oc.denoise(lambda *a: o(*a, image_rotary_emb=rope), oc.CogVideoXDDIMScheduler(), lat.half().float(), img, pe, dom, flow, 4,
                     6.0, True, callback=lambda i, t, l: ref_steps.append(l.clone()))
    got = pc.denoise(m, pc.CogVideoXDDIMScheduler(), lat.half().to(DEV), img.to(DEV), pe.to(DEV), dom.to(DEV), flow.to(DEV), 4, 6.0,
                     True, callback=lambda i, t, l: got_steps.append(l.clone()))
    assert len(got_steps) == len(ref_steps) == 4
    for i, (a, b) in enumerate(zip(got_steps, ref_steps)):
        print(f"step {i}: rel L2 {_rel(a, b):.3e}")
        assert _rel(a, b) < 2e-2, (i, _rel(a, b))
    assert _rel(got, ref) < 2e-2 and torch.isfinite(got.float()).all()


# ------------------------------------------------------------------------------------------------------------------- two ranks
def _tiny_rope_dit(dev):
    return hip_twin(ro.seeded_model(ro.TINY_ROPE_DIT, 4), ro.TINY_ROPE_DIT, dev)


def _worker_rope_dit(rank, world, port, q):
    """test_dist_gpu._worker_dit (dist_support.sharded_dit_loop) for the tiny rotary model.  World 2: the ranks are the CFG halves (each rotates the whole clip's
    rows); world 4: CFG halves x latent frames (2, 1) - a rank rotates its local q and k with the rows of its frames of the
    tables before the K gather, and adds its rows of the learned table"""
    from dist_support import sharded_dit_loop
    sharded_dit_loop(rank, world, port, _tiny_rope_dit, q)


@gpu
@pytest.mark.parametrize("world", [2, 4])
def test_sharded_rotary_dit_loop_equals_single_process(world):
    """against the single-process loop at test_sharded_dit_loop_equals_single_process's bound; world 4 is the one whose ranks hold
    frame slices"""
    from dist_support import run_world
    results = run_world(_worker_rope_dit, world)
    ref = [r["ref"] for r in results if "ref" in r][0]
    assert torch.isfinite(ref).all()
    for r in results:
        assert r["frame_shards"] == world // 2
        rel = ((r["out"] - ref).norm() / ref.norm()).item()
        assert rel <= 8e-3, f"rank {r['rank']}: sharded rotary DiT loop vs single process: relative L2 {rel:.3e}"

"""What the CogVideoX LoRA tests share (test_cogvideox_lora_cpu.py, test_cogvideox_lora_gpu.py): random adapters in the form
``save_lora_weights`` writes, the fp32 oracle holding ``W + c B A``, the plain HIP twin of an adapted model's packed weights, and the
derived bound on the fp32 fold.

The adapters: A ~ N(0, 1 / in_features), B ~ N(0, B_STD[rank]^2), both rounded to fp16 values; B is never zero.  ``B_STD`` is chosen so
that ``B A`` has about the size of the tiny oracle's attention weights: the fixture condition of the CPU tests - the fp32 oracle with
``W + c B A`` sits at least 0.1 relative L2 from the base oracle for every c the tests use - then holds with room."""
import copy

import torch

from cogvideox_support import DEV, dit_inputs, patchify

ATTN = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0")
ALL_SIX = ATTN + ("ff.net.0.proj", "ff.net.2")
#: std of B per rank: an element of B A then has std B_STD * sqrt(r / in_features), about 0.13 at the tiny model's 128 inputs (its
#: attention weights have std 0.088)
B_STD = {4: 0.75, 128: 0.14}
U32 = 2.0 ** -24                      # unit roundoff of fp32


def module_names(layers, targets):
    return [f"transformer_blocks.{i}.{t}" for i in range(layers) for t in targets]


def linear_shape(cfg, name):
    """(out_features, in_features) of a block linear of ``cfg``"""
    d = cfg.num_attention_heads * cfg.attention_head_dim
    if name.endswith("ff.net.0.proj"):
        return 4 * d, d
    if name.endswith("ff.net.2"):
        return d, 4 * d
    return d, d


def make_adapter(cfg, seed, rank, targets=ATTN, b_std=None):
    """{``<module>.lora_A.weight`` [r, in], ``<module>.lora_B.weight`` [out, r]}: peft's names without the adapter's (what
    ``get_peft_model_state_dict`` hands to ``save_lora_weights``), fp32 tensors holding fp16 values"""
    g = torch.Generator().manual_seed(seed)
    b_std = B_STD[rank] if b_std is None else b_std
    sd = {}
    for name in module_names(cfg.num_layers, targets):
        n_out, n_in = linear_shape(cfg, name)
        sd[f"{name}.lora_A.weight"] = (torch.randn(rank, n_in, generator=g) / n_in ** 0.5).half().float()
        sd[f"{name}.lora_B.weight"] = (b_std * torch.randn(n_out, rank, generator=g)).half().float()
    return sd


def with_prefix(sd, prefix="transformer."):
    return {prefix + k: v for k, v in sd.items()}


def delta(sd, name):
    """fp64 ``B A`` of one module of an adapter dict"""
    return sd[f"{name}.lora_B.weight"].double() @ sd[f"{name}.lora_A.weight"].double()


def folded_oracle(o, adapters):
    """a copy of the fp32 oracle ``o`` with ``W + sum c B A`` in every module the adapter dicts name; ``adapters``: [(dict, c)].  The
    sum is made in fp64 and stored in the oracle's fp32"""
    f = copy.deepcopy(o)
    params = dict(f.named_parameters())
    with torch.no_grad():
        for sd, c in adapters:
            for k in sd:
                if k.endswith(".lora_A.weight"):
                    name = k[: -len(".lora_A.weight")]
                    w = params[name + ".weight"]
                    w.copy_((w.double() + c * delta(sd, name)).float())
    return f


def swapped_qk(sd):
    """decoy: every to_q adapter on to_k and the reverse"""
    out = {}
    for k, v in sd.items():
        if ".to_q." in k:
            out[k.replace(".to_q.", ".to_k.")] = v
        elif ".to_k." in k:
            out[k.replace(".to_k.", ".to_q.")] = v
        else:
            out[k] = v
    return out


def crossed_layers(sd):
    """decoy: A of layer 0 with B of layer 1 and the reverse (2 layers)"""
    out = {}
    for k, v in sd.items():
        if ".lora_B." in k:
            other = k.replace("transformer_blocks.0.", "transformer_blocks.X.").replace("transformer_blocks.1.", "transformer_blocks.0.") \
                .replace("transformer_blocks.X.", "transformer_blocks.1.")
            out[other] = v
        else:
            out[k] = v
    return out


def oracle_forward(o, cfg, inputs=None):
    i = dit_inputs(cfg) if inputs is None else inputs
    with torch.no_grad():
        return o(i["hidden"], i["text"], i["t"], i["domain"], i["flow"])[0]


def hip_forward(m, cfg, inputs=None):
    i = dit_inputs(cfg) if inputs is None else inputs
    return m(i["hidden"].to(DEV), i["text"].to(DEV), i["t"].to(DEV), i["domain"].to(DEV), i["flow"].to(DEV), return_dict=False)[0]


def rows_call(m, cfg, batch=2):
    """a closure over one ``forward_rows`` call of the sin-cos tiny model (test_cogvideox_launches_gpu.py's arguments)"""
    i = dit_inputs(cfg, batch=batch)
    rows = patchify(i["hidden"].half()).to(DEV)
    F_, H, W = i["hidden"].shape[1], i["hidden"].shape[3], i["hidden"].shape[4]
    grid = (F_, H // 2, W // 2)
    text = m.fused_text(i["text"].to(DEV), i["domain"].to(DEV), i["flow"].to(DEV))
    return lambda: m.forward_rows(rows, grid, text, 721.0)


_PACK_SLOT = {"attn1.to_q": "q", "attn1.to_k": "k", "attn1.to_v": "v", "attn1.to_out.0": "o", "ff.net.0.proj": "f1", "ff.net.2": "f2"}


def packed_weight(m, name):
    """the fp16 [N, K] weight the packed model's GEMM reads for the block linear ``name`` (fp16 mode)"""
    _, i, rest = name.split(".", 2)
    return getattr(m.transformer_blocks[int(i)]._pk, _PACK_SLOT[rest])[0]


def twin_of(m, cfg, dev=DEV):
    """a plain model (no wrappers) whose state dict is the adapted, packed (fp16 mode) model ``m``'s with every wrapped linear's weight
    replaced by the packed folded weight"""
    from lkgd_amd import cogvideox as pc
    from lkgd_amd import lora
    assert m._pk is not None and not m._pk.fp8
    sd = {}
    for k, v in m.state_dict().items():
        if ".lora_A." in k or ".lora_B." in k:
            continue
        sd[k.replace(".base_layer.", ".")] = v.detach().clone()
    for name, _ in lora.lora_layers(m):
        sd[name + ".weight"] = packed_weight(m, name).detach().clone()
    t = pc.CogVideoXTransformer3DModel(pc.DiTConfig(**cfg.__dict__))
    missing, unexpected = t.load_state_dict(sd, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return t.half().to(dev)


# ------------------------------------------------------------------------------------------------------ the fold's bound
def gamma(n):
    """the relative error bound of n fp32 roundings"""
    return n * U32 / (1 - n * U32)


def fold_terms(w, a, b, c):
    """fp64 on the tensors' device: v = W + c B A and the magnitude sum |W| + |c| sum_j |B_nj| |A_jk|"""
    w, a, b = w.double(), a.double(), b.double()
    return w + c * (b @ a), w.abs() + abs(c) * (b.abs() @ a.abs())


def h(x):
    """fp64 -> fp16 values, as fp64.  The cast passes through fp32; the packed weight IS the fp16 rounding of an fp32 number x with
    lo <= x <= hi, and both roundings are monotone, so h(lo) <= packed <= h(hi) holds for this two-step h exactly as for a direct one"""
    return x.float().half().double()


def assert_within_fold_bound(packed, w, a, b, c, r):
    """for every element h(v - d) <= packed <= h(v + d), d = gamma(r + 2) (|W| + |c| sum_j |B_nj| |A_jk|): products of fp16 values are
    exact in fp32, and the fold performs at most r + 2 fp32 roundings per element (r in the product's sum, one for c, one for the add
    to W) in any order.  Returns how many elements differ from h(v) (informative)"""
    v, mag = fold_terms(w, a, b, c)
    d = gamma(r + 2) * mag
    p = packed.double()
    lo, hi = h(v - d), h(v + d)
    bad = ((p < lo) | (p > hi)).sum().item()
    assert bad == 0, (bad, p.numel(), float((p - v).abs().max()), float(d.max()))
    return (p != h(v)).sum().item()

"""Host side of the T5 text encoder without a GPU: the five entry points refuse bad arguments with the documented codes before any launch;
the module tree carries transformers' state-dict names and shapes; the relative-position table expands to transformers'
``compute_bias`` exactly; the configuration refusals name what they refuse; ``encode_prompt`` with a stub tokenizer and a stub
encoder.  transformers [EXT] is the checker, never on the product path."""
import pytest
import torch

transformers = pytest.importorskip("transformers")

from c_interface import ALIGN, NULL, SHAPE, Host, entry
from t5_support import TINY_A, StubTokenizer, expand_bias_table, hf_model, hip_twin


def test_t5_entry_points_refuse_before_launching():
    h = Host()
    embed = entry("lkgd_t5_embed_rows", ids=h.p, table=h.p, ldt=64, V=128, D=64, out=h.p, ldo=64, T=3)
    norm = entry("lkgd_t5_rmsnorm", x=h.p, ldx=64, T=3, C=64, weight=h.p, eps=1e-6, out=h.p, ldo=64)
    attn = entry("lkgd_attn_dense_relbias", q=h.p, ldq=192, k=h.p + 128, ldk=192, v=h.p + 256, ldv=192, out=h.p, ldo=64, nbatch=2, S=7,
                 heads=4, head_dim=16, relbias=h.p, scale=1.0)
    gelu = entry("lkgd_t5_gated_gelu", h=h.p, ldh=320, T=3, F=160, out=h.p, ldo=160)
    add = entry("lkgd_t5_residual_add", x=h.p, ldx=64, y=h.p, ldy=64, T=3, C=64, s=64.0)

    for k in ("ids", "table", "out"):
        assert embed(**{k: None}) == NULL, k
    for kw in (dict(T=0), dict(V=0), dict(D=0), dict(D=60), dict(ldt=56), dict(ldo=56)):
        assert embed(**kw) == SHAPE, kw
    for kw in (dict(table=h.p + 8), dict(out=h.p + 8), dict(ids=h.p + 4), dict(ldt=68), dict(ldo=66)):
        assert embed(**kw) == ALIGN, kw

    for k in ("x", "weight", "out"):
        assert norm(**{k: None}) == NULL, k
    for kw in (dict(T=0), dict(C=0), dict(C=60), dict(C=4104, ldx=4104, ldo=4104), dict(ldx=56), dict(ldo=56)):
        assert norm(**kw) == SHAPE, kw
    for kw in (dict(x=h.p + 8), dict(weight=h.p + 4), dict(out=h.p + 8), dict(ldx=66), dict(ldo=68)):
        assert norm(**kw) == ALIGN, kw

    for k in ("q", "k", "v", "out", "relbias"):
        assert attn(**{k: None}) == NULL, k
    for kw in (dict(nbatch=0), dict(S=0), dict(heads=0), dict(head_dim=0), dict(head_dim=12), dict(head_dim=136, heads=1),
               dict(S=4096), dict(ldq=56), dict(ldk=56), dict(ldv=56), dict(ldo=56)):
        assert attn(**kw) == SHAPE, kw
    # the table counts against the LDS bound.  At head_dim 8, K, V and the waves' rows take 56 S + 1024 bytes: S = 2907 is the last
    # length lkgd_attn_dense's bound of 160 KB admits; with the table's 8 S - 4 bytes on top it is refused here
    assert 56 * 2907 + 1024 <= 160 * 1024 < 56 * 2907 + 1024 + 8 * 2907 - 4
    assert attn(S=2907, heads=1, head_dim=8, ldq=8, ldk=8, ldv=8, ldo=8) == SHAPE
    for kw in (dict(q=h.p + 8), dict(k=h.p + 8), dict(v=h.p + 8), dict(out=h.p + 2), dict(relbias=h.p + 2), dict(ldq=196), dict(ldk=196),
               dict(ldv=196), dict(ldo=65)):
        assert attn(**kw) == ALIGN, kw

    for k in ("h", "out"):
        assert gelu(**{k: None}) == NULL, k
    for kw in (dict(T=0), dict(F=0), dict(F=156), dict(ldh=312), dict(ldo=152)):
        assert gelu(**kw) == SHAPE, kw
    for kw in (dict(h=h.p + 8), dict(out=h.p + 8), dict(ldh=324), dict(ldo=164)):
        assert gelu(**kw) == ALIGN, kw

    for k in ("x", "y"):
        assert add(**{k: None}) == NULL, k
    for kw in (dict(T=0), dict(C=0), dict(C=60), dict(ldx=56), dict(ldy=56)):
        assert add(**kw) == SHAPE, kw
    for kw in (dict(x=h.p + 8), dict(y=h.p + 8), dict(ldx=66), dict(ldy=68)):
        assert add(**kw) == ALIGN, kw
    assert add(x=None, C=60) == NULL                                       # NULL comes first


def test_state_dict_names_and_shapes_are_transformers():
    from lkgd_amd import t5
    ref = hf_model(TINY_A)
    ours = t5.T5EncoderModel(t5.T5Config(**TINY_A))
    want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert {k: tuple(v.shape) for k, v in ours.state_dict().items()} == want
    for k in ("shared.weight", "encoder.embed_tokens.weight", "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight",
              "encoder.block.1.layer.1.DenseReluDense.wi_1.weight", "encoder.final_layer_norm.weight"):
        assert k in want
    assert "encoder.block.1.layer.0.SelfAttention.relative_attention_bias.weight" not in want
    r = ours.load_state_dict(ref.state_dict(), strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    for k, v in ref.state_dict().items():
        assert torch.equal(ours.state_dict()[k], v), k
    assert ours.encoder.embed_tokens.weight is ours.shared.weight


def test_tied_embedding_key_is_accepted_or_refused(tmp_path):
    from lkgd_amd import t5
    from lkgd_amd._lib import LkgdHipError
    ref = hf_model(TINY_A)
    sd = dict(ref.state_dict())
    for drop in ("encoder.embed_tokens.weight", "shared.weight"):          # either name alone carries the tensor
        ours = t5.T5EncoderModel(t5.T5Config(**TINY_A))
        r = ours.load_state_dict({k: v for k, v in sd.items() if k != drop}, strict=True)
        assert not r.missing_keys and not r.unexpected_keys and torch.equal(ours.shared.weight, sd["shared.weight"])
    bad = dict(sd)
    bad["encoder.embed_tokens.weight"] = sd["shared.weight"] + 1
    with pytest.raises(LkgdHipError, match="encoder.embed_tokens.weight"):
        t5.T5EncoderModel(t5.T5Config(**TINY_A)).load_state_dict(bad)
    with pytest.raises(RuntimeError, match="wi_0"):                        # every key is checked
        t5.T5EncoderModel(t5.T5Config(**TINY_A)).load_state_dict(
            {k: v for k, v in sd.items() if k != "encoder.block.1.layer.1.DenseReluDense.wi_0.weight"}, strict=True)
    # save_pretrained -> from_pretrained: config.json + one safetensors file without the tied copy
    ours = hip_twin(ref, TINY_A)
    ours._pk = object()
    ours.save_pretrained(str(tmp_path / "text_encoder"))
    back = t5.T5EncoderModel.from_pretrained(str(tmp_path), torch_dtype=torch.float32)
    assert back.config == ours.config and back.dtype == torch.float32 and back._pk is None
    for k, v in ours.state_dict().items():
        assert torch.equal(back.state_dict()[k], v), k
    half = t5.T5EncoderModel.from_pretrained(str(tmp_path))
    assert half.dtype == torch.float16 and half.encoder.embed_tokens.weight is half.shared.weight
    ours.half()
    assert ours._pk is None                                                # _apply forgets the packed weights


@pytest.mark.parametrize("S", [1, 7, 129, 226, 300])
def test_bias_table_expands_to_compute_bias(S):
    """[heads, 2S - 1] -> exactly transformers' compute_bias(S, S): sequence lengths on both sides of max_distance = 128"""
    ref = hf_model(TINY_A)
    ours = hip_twin(ref, TINY_A)
    table = ours.bias_table(S)
    assert table.dtype == torch.float32 and tuple(table.shape) == (TINY_A["num_heads"], 2 * S - 1) and table.is_contiguous()
    assert ours.bias_table(S) is table                                      # cached per S
    with torch.no_grad():
        want = ref.encoder.block[0].layer[0].SelfAttention.compute_bias(S, S)
    assert torch.equal(expand_bias_table(table, S), want)
    if S > 1:                                                               # not symmetric: j - i and i - j differ
        assert not torch.equal(table, table.flip(1))


def test_config_refusals_name_what_they_refuse():
    from lkgd_amd import t5
    from lkgd_amd._lib import LkgdHipError
    for over, word in ((dict(feed_forward_proj="relu"), "feed_forward_proj 'relu'"), (dict(feed_forward_proj="gated-silu"), "gated-silu"),
                       (dict(d_model=4104), "d_model 4104"), (dict(d_kv=12), "d_kv 12"), (dict(d_kv=136), "d_kv 136"),
                       (dict(num_heads=3), "num_heads")):
        with pytest.raises(LkgdHipError, match=word):
            t5.T5EncoderModel(t5.T5Config(**{**TINY_A, **over}))
    m = t5.T5EncoderModel(t5.T5Config(**TINY_A))
    ids = torch.zeros(1, 7, dtype=torch.int64)
    with pytest.raises(LkgdHipError, match="attention_mask"):
        m(ids, attention_mask=torch.ones(1, 7))
    with pytest.raises(ValueError, match=r"\[0, 128\)"):
        m(torch.full((1, 7), 128, dtype=torch.int64))
    with pytest.raises(LkgdHipError, match="cuda"):                        # no CPU path: the refusal, not a fallback
        m(ids)
    c = t5.T5Config()                                                       # the defaults are the XXL encoder of CogVideoX
    assert (c.d_model, c.d_kv, c.d_ff, c.num_layers, c.num_heads, c.vocab_size) == (4096, 64, 10240, 24, 64, 32128)
    t5.check_t5_config(c)


# ------------------------------------------------------------------------------------------------------------ encode_prompt
class _StubEncoder:
    """embeds id i as the row [i, i + 0.5, ...]: the result shows which ids went in, in which order"""
    device, dtype = torch.device("cpu"), torch.float16

    def __init__(self, d=8):
        self.d, self.seen = d, []

    def __call__(self, ids):
        self.seen.append(ids.clone())
        return (ids[..., None].to(torch.float16) + 0.5 * torch.arange(self.d, dtype=torch.float16),)


def test_encode_prompt_shapes_defaults_and_errors():
    import inspect
    from lkgd_amd import cogvideox as pc
    from lkgd_amd._lib import LkgdHipError
    sig = inspect.signature(pc.encode_prompt)
    assert list(sig.parameters) == ["text_encoder", "tokenizer", "prompt", "negative_prompt", "do_classifier_free_guidance",
                                    "num_videos_per_prompt", "prompt_embeds", "negative_prompt_embeds", "max_sequence_length", "device",
                                    "dtype"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d["negative_prompt"], d["do_classifier_free_guidance"], d["num_videos_per_prompt"], d["max_sequence_length"]) == \
        (None, True, 1, 226)
    enc, tok = _StubEncoder(), StubTokenizer()
    pe, ne = pc.encode_prompt(enc, tok, ["a cat", "two dogs"], num_videos_per_prompt=2)
    assert pe.shape == ne.shape == (4, 226, 8) and pe.dtype == ne.dtype == torch.float16
    # the reference's repeat(1, n, 1).view(B * n, S, -1): each prompt's copies are adjacent
    assert torch.equal(pe[0], pe[1]) and torch.equal(pe[2], pe[3]) and not torch.equal(pe[0], pe[2])
    assert [c["prompt"] for c in tok.calls] == [["a cat", "two dogs"], ["", ""]]           # the negative default: "" per prompt
    assert all(c["max_length"] == 226 for c in tok.calls)
    assert ne[0, 0, 0].item() == 1.0 and bool((ne[:, 1:, 0] == 0).all())                   # "" = </s> then padding
    assert pe[0, 0, 0].item() == 2 + ord("a") and pe[0, 5, 0].item() == 1.0
    # a string is one prompt; without guidance no negative is encoded
    pe1, ne1 = pc.encode_prompt(enc, tok, "a cat", do_classifier_free_guidance=False, max_sequence_length=16)
    assert pe1.shape == (1, 16, 8) and ne1 is None and torch.equal(pe1[0, :6], pe[0, :6])
    # ids in place of text; given embeddings pass through
    ids = torch.arange(2 * 9, dtype=torch.int64).reshape(2, 9) % 100
    pe2, ne2 = pc.encode_prompt(enc, None, ids, negative_prompt=ids.flip(0), num_videos_per_prompt=1)
    assert torch.equal(pe2[..., 0], ids.to(torch.float16)) and torch.equal(ne2[..., 0], ids.flip(0).to(torch.float16))
    pe3, ne3 = pc.encode_prompt(enc, tok, None, prompt_embeds=pe2, negative_prompt_embeds=ne2)
    assert pe3 is pe2 and ne3 is ne2
    with pytest.raises(LkgdHipError, match="tokenizer"):
        pc.encode_prompt(enc, None, "a cat")
    # the two reference error branches, in its words
    with pytest.raises(TypeError, match="`negative_prompt` should be the same type to `prompt`"):
        pc.encode_prompt(enc, tok, ["a cat"], negative_prompt=("a", ))
    with pytest.raises(ValueError, match="has batch size 2, but `prompt`"):
        pc.encode_prompt(enc, tok, ["a cat"], negative_prompt=["x", "y"])

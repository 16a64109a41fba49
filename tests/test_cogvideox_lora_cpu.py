"""LoRA adapters on the CogVideoX DiT, the part that needs no GPU: key handling, the ``save_lora_weights`` round trip, peft's state-dict
names, the ``quaternion_lora_*`` tensors of a LoRA file, the scale bookkeeping of the reference's two call sequences
(inference/cli_demo.py:128-132, tools/load_cogvideox_lora.py:91-98) and the fuse / unfuse / unload transitions - all on a CPU module,
the order cli_demo.py uses (adapters first, ``.to("cuda")`` after).  Plus the condition on the tests' own adapters: they move the fp32
oracle by at least ten times the forward gate."""
import logging

import pytest
import torch

import cogvideox_lora_support as ls
from cogvideox_support import hip_twin, rel, tiny_oracle

R_TRAINER, ALPHA_TRAINER = 128, 64          # finetune/schemas/args.py:75-77


@pytest.fixture(scope="module")
def cfg():
    from oracle import cogvideox as oc
    return oc.TINY_DIT


@pytest.fixture(scope="module")
def oracle():
    return tiny_oracle()


@pytest.fixture(scope="module")
def adapters(cfg):
    return {4: ls.make_adapter(cfg, 904, 4), 128: ls.make_adapter(cfg, 1028, 128), "six": ls.make_adapter(cfg, 906, 4, ls.ALL_SIX)}


def _pipe(oracle):
    """a pipeline around a CPU DiT alone: the LoRA surface touches no other component"""
    from lkgd_amd.pipeline_cogvideox import CogVideoXImageToVideoPipeline
    return CogVideoXImageToVideoPipeline(None, None, None, hip_twin(oracle), None)


def _base_weights(m):
    from lkgd_amd import lora
    wrapped = dict(lora.lora_layers(m))
    return {n: (wrapped[n].base_layer.weight if n in wrapped else m.get_submodule(n).weight).detach().clone()
            for n in ls.module_names(2, ls.ALL_SIX)}


# ------------------------------------------------------------------------------------------------------- fixture condition
@pytest.mark.parametrize("rank, c, targets", [(4, 0.5, "attn"), (128, 0.5, "attn"), (128, 1.0, "attn"), (4, 0.75, "six")])
def test_adapters_move_the_oracle_by_ten_gates(cfg, oracle, adapters, rank, c, targets):
    """B is not zero, and the fp32 oracle with W + c B A is at least 0.1 relative L2 from the base oracle on ``dit_inputs``"""
    sd = adapters["six"] if targets == "six" else adapters[rank]
    assert all(v.abs().max() > 0 for k, v in sd.items() if ".lora_B." in k)
    assert all(torch.equal(v, v.half().float()) for v in sd.values())
    sep = rel(ls.oracle_forward(ls.folded_oracle(oracle, [(sd, c)]), cfg), ls.oracle_forward(oracle, cfg))
    print(f"\noracle separation rank {rank} c {c} {targets}: rel L2 {sep:.3f}")
    assert sep >= 0.1


# ------------------------------------------------------------------------------------------------------------ key handling
def test_lora_state_dict_strips_the_prefix_and_reads_ranks(oracle, adapters):
    from lkgd_amd import lora
    from lkgd_amd.pipeline_cogvideox import CogVideoXImageToVideoPipeline as P
    mixed = {**ls.with_prefix(adapters[4]), **{k: v for k, v in adapters[128].items() if "blocks.1.attn1.to_v" in k}}
    sd = P.lora_state_dict(mixed)
    assert set(sd) == set(adapters[4]) and not any(k.startswith("transformer.") for k in sd)
    assert P.lora_state_dict(sd).keys() == sd.keys()                          # its own output passes through
    pipe = _pipe(oracle)
    absent = pipe.load_lora_weights(mixed)                                    # rank 4 everywhere, rank 128 on one module
    assert pipe.get_active_adapters() == ["default_0"]
    layers = dict(lora.lora_layers(pipe.transformer))
    assert sorted(layers) == sorted(ls.module_names(2, ls.ATTN))
    for n, m in layers.items():
        r = 128 if n == "transformer_blocks.1.attn1.to_v" else 4
        assert m.r == {"default_0": r} and m.lora_alpha == {"default_0": r} and m.scaling == {"default_0": 1.0}, n
        assert tuple(m.lora_A["default_0"].weight.shape) == (r, 128) and tuple(m.lora_B["default_0"].weight.shape) == (128, r)
    assert absent == sorted(k for k in pipe.transformer.state_dict() if k.startswith("quaternion_lora_"))
    pipe.load_lora_weights(adapters[128])
    assert lora.adapter_names(pipe.transformer) == ["default_0", "default_1"] and pipe.get_active_adapters() == ["default_1"]


def test_bad_keys_raise_and_name_themselves(oracle, adapters):
    from lkgd_amd import LkgdHipError
    from lkgd_amd import lora
    good = adapters[4]
    pipe = _pipe(oracle)
    stock = set(pipe.transformer.state_dict())

    def refused(sd, name, exc=(LkgdHipError, ValueError), **kw):
        with pytest.raises(exc) as e:
            pipe.load_lora_weights(sd, **kw)
        assert name in str(e.value), str(e.value)
        assert set(pipe.transformer.state_dict()) == stock and not lora.lora_layers(pipe.transformer)     # nothing half-loaded

    a, b = good["transformer_blocks.0.attn1.to_q.lora_A.weight"], good["transformer_blocks.0.attn1.to_q.lora_B.weight"]
    for other in ("transformer_blocks.0.norm1.linear", "patch_embed.text_proj", "proj_out", "transformer_blocks.0.attn1.to_x",
                  "transformer_blocks.7.attn1.to_q"):
        refused({**good, f"transformer.{other}.lora_A.weight": a, f"transformer.{other}.lora_B.weight": b}, other)
    refused({**good, "text_encoder.encoder.block.0.layer.0.SelfAttention.q.lora_A.weight": a}, "text_encoder.encoder.block.0")
    refused({**good, "transformer_blocks.1.attn1.to_k.lora_B.weight": torch.zeros(64, 4)}, "transformer_blocks.1.attn1.to_k")
    refused({**good, "transformer_blocks.1.ff.net.2.lora_A.weight": a, "transformer_blocks.1.ff.net.2.lora_B.weight": b},
            "transformer_blocks.1.ff.net.2")                                 # A [4, 128] does not fit the 512 inputs
    refused({k: v for k, v in good.items() if not k.endswith("0.attn1.to_v.lora_B.weight")}, "transformer_blocks.0.attn1.to_v")
    refused({**good, "transformer_blocks.0.attn1.to_q.alpha": torch.tensor(8.0)}, "transformer_blocks.0.attn1.to_q.alpha")
    refused({**good, "transformer_blocks.0.attn1.to_q.weight": a}, "transformer_blocks.0.attn1.to_q.weight")
    # a duplicate adapter name
    pipe.load_lora_weights(good, adapter_name="kite")
    with pytest.raises(ValueError, match="kite"):
        pipe.load_lora_weights(good, adapter_name="kite")
    # components other than the transformer, unknown adapters
    for call in (lambda: pipe.fuse_lora(components=["transformer", "text_encoder"]), lambda: pipe.unfuse_lora(components=["vae"])):
        with pytest.raises(LkgdHipError, match="text_encoder|vae"):
            call()
    with pytest.raises(ValueError, match="gull"):
        pipe.set_adapters(["gull"])
    with pytest.raises(ValueError, match="gull"):
        pipe.fuse_lora(adapter_names=["gull"])


# -------------------------------------------------------------------------------------------------------------- round trip
@pytest.mark.parametrize("safe", [True, False])
def test_save_then_load_round_trip(tmp_path, oracle, adapters, safe):
    from lkgd_amd import lora
    pipe = _pipe(oracle)
    g = torch.Generator().manual_seed(3)
    texts = torch.randn(256, generator=g)
    pipe.load_lora_weights(adapters["six"], adapter_name="a")
    layers = {**lora.adapter_state_dict(pipe.transformer, "a"), "quaternion_lora_texts": texts}
    assert set(layers) == set(adapters["six"]) | {"quaternion_lora_texts"}
    name = "pytorch_lora_weights.safetensors" if safe else "pytorch_lora_weights.bin"
    pipe.save_lora_weights(str(tmp_path), transformer_lora_layers=layers, weight_name=name, safe_serialization=safe)
    assert (tmp_path / name).is_file()
    for source in (str(tmp_path), str(tmp_path / name)):                      # a directory, a file
        sd = pipe.lora_state_dict(source, weight_name=name)
        assert set(sd) == set(layers) and all(torch.equal(sd[k], layers[k]) for k in layers)
    other = _pipe(oracle)
    other.load_lora_weights(str(tmp_path), weight_name=name, adapter_name="b")
    got = lora.adapter_state_dict(other.transformer, "b")
    assert set(got) == set(adapters["six"]) and all(torch.equal(got[k], adapters["six"][k]) for k in got)
    assert torch.equal(other.transformer.quaternion_lora_texts.detach(), texts)
    with pytest.raises(FileNotFoundError):
        pipe.lora_state_dict(str(tmp_path), weight_name="absent.safetensors")


# -------------------------------------------------------------------------------------------------------- state-dict names
def test_state_dict_names_are_pefts_while_loaded_and_stock_after_unload(oracle, adapters):
    pipe = _pipe(oracle)
    stock = list(pipe.transformer.state_dict())
    pipe.load_lora_weights(adapters[4], adapter_name="kite")
    names = set(pipe.transformer.state_dict())
    for n in ls.module_names(2, ls.ATTN):
        assert {f"{n}.base_layer.weight", f"{n}.base_layer.bias", f"{n}.lora_A.kite.weight", f"{n}.lora_B.kite.weight"} <= names
        assert f"{n}.weight" not in names
    assert "transformer_blocks.0.ff.net.2.weight" in names                    # not targeted: not wrapped
    pipe.unload_lora_weights()
    assert list(pipe.transformer.state_dict()) == stock
    assert pipe.get_active_adapters() == []


# ------------------------------------------------------------------------------------------------- quaternion_lora_* keys
def test_quaternion_keys_present_replace_absent_are_reported(oracle, adapters, caplog):
    from lkgd_amd import LkgdHipError
    pipe = _pipe(oracle)
    m = pipe.transformer
    before = {k: v.detach().clone() for k, v in m.state_dict().items() if k.startswith("quaternion_lora_")}
    g = torch.Generator().manual_seed(4)
    given = {k: torch.randn(before[k].shape, generator=g) for k in ("quaternion_lora_texts", "quaternion_lora_dconv.weight",
                                                                    "quaternion_lora_fuse_sf.2.bias")}
    m._pk = object()
    with caplog.at_level(logging.WARNING, logger="lkgd_amd.cogvideox"):
        absent = pipe.load_lora_weights({**ls.with_prefix(adapters[4]), **ls.with_prefix(given)})
    assert m._pk is None
    assert absent == sorted(set(before) - set(given)) and len(absent) == len(before) - 3
    records = [r for r in caplog.records if "quaternion_lora_" in r.getMessage()]
    assert len(records) == 1 and all(k in records[0].getMessage() for k in absent)        # logged once, every name
    after = m.state_dict()
    for k in before:
        assert torch.equal(after[k], given[k] if k in given else before[k]), k
    # a wrong shape and an unknown name raise, naming the key, and leave everything as it is
    snapshot = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for bad, exc in (({"transformer.quaternion_lora_texts": torch.zeros(255)}, ValueError),
                     ({"transformer.quaternion_lora_nothing": torch.zeros(3)}, LkgdHipError)):
        with pytest.raises(exc, match=next(iter(bad))[len("transformer."):]):
            pipe.load_lora_weights({**ls.with_prefix(adapters[128]), **bad})
        now = m.state_dict()
        assert set(now) == set(snapshot) and all(torch.equal(now[k], snapshot[k]) for k in now)
    # a file holding only such tensors loads them and adds no adapter
    pipe.load_lora_weights({"transformer.quaternion_lora_texts_fft_mag": torch.ones(129)})
    assert torch.equal(m.quaternion_lora_texts_fft_mag.detach(), torch.ones(129)) and pipe.get_active_adapters() == ["default_0"]


# -------------------------------------------------------------------------------------------------------- scale bookkeeping
def _cs(pipe):
    """the distinct c per adapter over all wrapped modules"""
    out = {}
    for per in pipe.transformer.lora_coefficients().values():
        for a, c in per.items():
            out.setdefault(a, set()).add(c)
    return out


def test_both_reference_sequences_leave_the_expected_c(oracle, adapters):
    """cli_demo.py:128-132 fuses at lora_scale 1.0; load_cogvideox_lora.py:91-98 weights the adapter by lora_alpha / lora_r.  A file
    of ``save_lora_weights`` has no alpha entries: lora_alpha = r, so those two numbers ARE c"""
    pipe = _pipe(oracle)
    pipe.load_lora_weights(adapters[128], weight_name="pytorch_lora_weights.safetensors", adapter_name="test_1")
    pipe.fuse_lora(components=["transformer"], lora_scale=1.0)
    assert _cs(pipe) == {"test_1": {1.0}} and pipe.get_active_adapters() == ["test_1"]

    pipe = _pipe(oracle)
    pipe.load_lora_weights(adapters[128], weight_name="pytorch_lora_weights.safetensors", adapter_name="cogvideox-lora")
    pipe.set_adapters(["cogvideox-lora"], [ALPHA_TRAINER / R_TRAINER])
    assert _cs(pipe) == {"cogvideox-lora": {0.5}} and pipe.get_active_adapters() == ["cogvideox-lora"]


def test_c_is_weight_times_fuse_scale_times_alpha_over_r(oracle, adapters):
    from lkgd_amd import lora
    pipe = _pipe(oracle)
    m = pipe.transformer
    pipe.load_lora_weights(adapters[4], adapter_name="a")
    pipe.load_lora_weights(adapters[128], adapter_name="b")
    assert _cs(pipe) == {"b": {1.0}}                                          # the adapter loaded last is the active one
    pipe.set_adapters(["a", "b"], [0.5, 1.5])
    assert _cs(pipe) == {"a": {0.5}, "b": {1.5}} and pipe.get_active_adapters() == ["a", "b"]
    pipe.fuse_lora(lora_scale=0.5, adapter_names=["b"])                      # fused: the fused adapters alone act
    assert _cs(pipe) == {"b": {0.75}} and pipe.get_active_adapters() == ["b"]
    pipe.set_adapters(["a", "b"], [0.5, 1.0])
    assert _cs(pipe) == {"b": {0.5}}
    pipe.unfuse_lora()
    assert _cs(pipe) == {"a": {0.5}, "b": {1.0}}
    # an alpha other than r enters as alpha / r (lora.add_adapter: what an `.alpha` entry would set)
    lora.add_adapter(m, "c", r=4, lora_alpha=3.0, target_modules=["transformer_blocks.0.attn1.to_q"], init_lora_weights=False)
    pipe.set_adapters(["c"], [2.0])
    pipe.fuse_lora(lora_scale=0.5)
    assert m.lora_coefficients()["transformer_blocks.0.attn1.to_q"] == {"c": 2.0 * 0.5 * 3.0 / 4}
    pipe.disable_lora()
    assert _cs(pipe) == {} and pipe.get_active_adapters() == []
    pipe.enable_lora()
    assert _cs(pipe) == {"c": {0.75}}
    with pytest.raises(Exception, match="fused already"):
        pipe.fuse_lora(lora_scale=0.5)


# ------------------------------------------------------------------------------------------------------ fuse, unfuse, unload
def _transition(m, call):
    """every state change forgets the pack"""
    m._pk = object()
    out = call()
    assert m._pk is None
    return out


def test_fuse_unfuse_unload_transitions(oracle, adapters):
    sd, c = adapters["six"], 0.75
    pipe = _pipe(oracle)
    m = pipe.transformer
    w0 = _base_weights(m)
    _transition(m, lambda: pipe.load_lora_weights(sd, adapter_name="a"))
    _transition(m, lambda: pipe.set_adapters(["a"], [1.5]))
    _transition(m, lambda: pipe.fuse_lora(lora_scale=0.5))
    assert all(torch.equal(v, w0[n]) for n, v in _base_weights(m).items())          # fused: the base is not written
    _transition(m, pipe.unfuse_lora)
    assert all(torch.equal(v, w0[n]) for n, v in _base_weights(m).items())          # fuse then unfuse: bit-identical
    _transition(m, pipe.disable_lora)
    _transition(m, pipe.enable_lora)

    # plain unload: base untouched
    _transition(m, pipe.unload_lora_weights)
    assert all(torch.equal(v, w0[n]) for n, v in _base_weights(m).items())
    assert all(torch.equal(v, oracle.state_dict()[k]) for k, v in m.state_dict().items())

    # fuse then unload: base = h(fp32 fold)
    pipe.load_lora_weights(sd, adapter_name="a")
    pipe.fuse_lora(lora_scale=c)
    _transition(m, pipe.unload_lora_weights)
    got = _base_weights(m)
    for n in ls.module_names(2, ls.ALL_SIX):
        a, b = sd[f"{n}.lora_A.weight"], sd[f"{n}.lora_B.weight"]
        want = (w0[n].float() + (b.float() @ a.float()) * c).half().float()
        assert torch.equal(got[n], want), n
        ls.assert_within_fold_bound(got[n], w0[n], a, b, c, 4)
        assert not torch.equal(got[n], w0[n])
    assert list(m.state_dict()) == list(oracle.state_dict())


def test_half_module_on_the_cpu_then_prepare_needs_the_gpu(oracle, adapters):
    """the order of cli_demo.py: adapters on a CPU module; only ``prepare()`` asks for the GPU"""
    from lkgd_amd import LkgdHipError
    pipe = _pipe(oracle)
    pipe.transformer.half()
    pipe.load_lora_weights(adapters[4])
    pipe.fuse_lora(lora_scale=0.5)
    assert all(p.dtype == torch.float16 for p in pipe.transformer.parameters())
    with pytest.raises(LkgdHipError, match="cuda"):
        pipe.transformer.prepare()
    with pytest.raises(LkgdHipError, match="attention_kwargs"):
        pipe._not_built(None, 0.0, {"scale": 0.5})

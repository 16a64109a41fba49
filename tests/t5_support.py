"""What the T5 tests share (test_t5_cpu.py, test_t5_gpu.py): the two tiny configurations, transformers' ``T5EncoderModel`` [EXT] at
them with fp16-rounded random weights (the checker: its fp32 CPU forward), the HIP twin holding the same weights, and stub
tokenizers.  transformers is never on the product path; both test files skip where it is absent."""
from types import SimpleNamespace

import torch

DEV = "cuda:0"
GATE = 1e-2                         # relative L2: the project's gate for clip.py against transformers and the DiT against its oracle
BIAS_STD = 2.0                      # standard deviation of the relative-position table: separates the decoys (test_t5_gpu.py)

#: d_model 64, 4 heads of 16, d_ff 160 (not a multiple of 64: the packed feed-forward is padded), 2 layers, vocab 128
TINY_A = dict(vocab_size=128, d_model=64, d_kv=16, d_ff=160, num_layers=2, num_heads=4)
#: d_model 128, 2 heads of 64 (the released head width), d_ff 320, 3 layers
TINY_B = dict(vocab_size=128, d_model=128, d_kv=64, d_ff=320, num_layers=3, num_heads=2)
TINY = {"a": TINY_A, "b": TINY_B}


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def expand_bias_table(table: torch.Tensor, S: int) -> torch.Tensor:
    """[heads, 2S - 1] -> [1, heads, S, S], the layout of transformers' ``compute_bias``: entry [h, i, j] = table[h, j - i + S - 1]"""
    i = torch.arange(S, device=table.device)
    return table[:, (i[None, :] - i[:, None]) + S - 1][None]


def hf_model(cfg: dict, seed: int = 3, bias_std: float = BIAS_STD):
    """transformers' fp32 encoder at ``cfg``: seeded random weights rounded to fp16 values, norm weights off one, the
    relative-position table drawn with ``bias_std``"""
    import transformers
    torch.manual_seed(seed)
    c = transformers.T5Config(feed_forward_proj="gated-gelu", **cfg)
    m = transformers.T5EncoderModel(c).float().eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("layer_norm.weight"):
                p.uniform_(0.7, 1.3)
            elif "relative_attention_bias" in n:
                p.normal_(0, bias_std)
            elif n == "shared.weight":
                p.normal_(0, 1.0)
            else:                                    # linears: outputs of about unit size at every width
                p.normal_(0, p.shape[1] ** -0.5)
        for p in m.parameters():
            p.copy_(p.half().float())
    return m


def hip_twin(ref, cfg: dict, dev=None):
    """``lkgd_amd.t5.T5EncoderModel`` holding ``ref``'s weights, every key checked; fp32 on the CPU, or fp16 on ``dev``"""
    from lkgd_amd import t5
    m = t5.T5EncoderModel(t5.T5Config(**cfg))
    missing, unexpected = m.load_state_dict(ref.state_dict(), strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return m if dev is None else m.half().to(dev)


def ids_for(cfg: dict, B: int, S: int, seed: int = 5) -> torch.Tensor:
    """int64 [B, S]: random ids, then the pad id 0 to the end as a tokenizer pads (padding is attended: there is no mask)"""
    g = torch.Generator().manual_seed(seed + S)
    ids = torch.randint(2, cfg["vocab_size"], (B, S), generator=g)
    for b in range(B):
        n = max(1, S - (b + 1) * (S // 3))
        ids[b, n - 1] = 1                            # </s>
        ids[b, n:] = 0
    return ids


class StubTokenizer:
    """callable as the reference calls its tokenizer: bytes of the text modulo the vocabulary, </s>, padding 0; records its calls"""

    def __init__(self, vocab_size: int = 128):
        self.vocab_size, self.calls = vocab_size, []

    def __call__(self, prompt, padding=None, max_length=None, truncation=None, add_special_tokens=None, return_tensors=None):
        self.calls.append(dict(prompt=list(prompt), padding=padding, max_length=max_length, truncation=truncation,
                               add_special_tokens=add_special_tokens, return_tensors=return_tensors))
        assert padding == "max_length" and truncation is True and add_special_tokens is True and return_tensors == "pt"
        ids = torch.zeros(len(prompt), max_length, dtype=torch.int64)
        for b, text in enumerate(prompt):
            toks = [2 + (c % (self.vocab_size - 2)) for c in text.encode()][:max_length - 1] + [1]
            ids[b, :len(toks)] = torch.tensor(toks)
        return SimpleNamespace(input_ids=ids)

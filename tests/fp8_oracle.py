"""Test-side restatement of the FP8 mode (include/lkgd_hip_fp8.h, lkgd_amd/fp8.py), independent of both: the e4m3fn value table from
the format's definition, round-to-nearest-even by searching that table in float64, the quantisation statement Q, the fake-quant
linear and the "twin" - a deep copy of an fp32 oracle DiT whose six block linears are replaced by

    x.half().float() -> Q per row -> decoded matmul in fp32 against the Q weight rows -> x scales -> + bias.

Nothing here uses torch's float8 dtypes except ``torch_cast`` (the cross-check the CPU test runs once)."""
import copy

import torch
import torch.nn as nn

E4M3_MAX = 448.0
#: |value| of the bytes 0x00 .. 0x7E (bias 7, three mantissa bits, subnormals below 2^-6); 0x7F is NaN
TABLE = torch.tensor([(b & 7) * 2.0 ** -9 if b >> 3 == 0 else (1 + (b & 7) / 8.0) * 2.0 ** ((b >> 3) - 7) for b in range(127)],
                     dtype=torch.float64)
BLOCK_LINEARS = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "ff.net.0.proj", "ff.net.2")


def decode(q: torch.Tensor) -> torch.Tensor:
    """uint8 e4m3fn bytes -> fp32 values (NaN for 0x7F / 0xFF)"""
    q = q.cpu().to(torch.int64)
    mag = q & 0x7F
    v = torch.where(mag == 0x7F, torch.full((), float("nan"), dtype=torch.float64), TABLE[mag.clamp(max=126)])
    return torch.where((q & 0x80) != 0, -v, v).to(torch.float32)


def rne_e4m3(v: torch.Tensor) -> torch.Tensor:
    """fp32 values with |v| <= 448 -> bytes: the nearest table entry, a tie to the entry with an even byte"""
    a = v.abs().to(torch.float64)
    assert bool((a <= E4M3_MAX).all())
    hi = torch.searchsorted(TABLE, a.contiguous()).clamp(max=126)          # first entry >= a
    lo = (hi - 1).clamp(min=0)
    d_hi, d_lo = TABLE[hi] - a, a - TABLE[lo]
    pick_hi = (d_hi < d_lo) | ((d_hi == d_lo) & (hi % 2 == 0))
    b = torch.where(pick_hi, hi, lo)
    return (b | torch.where(torch.signbit(v), 0x80, 0)).to(torch.uint8)


def q_rows(x: torch.Tensor):
    """the statement Q on every row of ``x`` [T, K] (fp16 values; taken as fp32) -> (bytes uint8 [T, K], scale fp32 [T])"""
    x = x.cpu().to(torch.float16).to(torch.float32)
    amax = x.abs().amax(dim=1)
    inv, scale = torch.ones_like(amax), torch.ones_like(amax)
    nz = amax > 0
    inv[nz] = torch.tensor(E4M3_MAX, dtype=torch.float32) / amax[nz]          # fp32 divisions, correctly rounded on the host
    scale[nz] = amax[nz] / torch.tensor(E4M3_MAX, dtype=torch.float32)
    p = (x * inv[:, None]).clamp(-E4M3_MAX, E4M3_MAX)                         # one fp32 rounding, then the explicit clamp
    return rne_e4m3(p), scale


def torch_cast(x: torch.Tensor) -> torch.Tensor:
    """torch's own fp32 -> float8_e4m3fn cast after the clamp (round to nearest even on the host): the yardstick of ``rne_e4m3``"""
    return x.clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8)


def special_rows(K: int, seed: int = 5) -> torch.Tensor:
    """fp16 [8, K]: random rows of three magnitudes, a zero row, rows with one +65504 / -65504, a row of fp16 subnormals (both signs),
    a row with signed zeros between values"""
    g = torch.Generator().manual_seed(seed + K)
    r = torch.randn(8, K, generator=g)
    r[1] *= 40.0
    r[2] *= 1e-3
    r[3] = 0.0
    r[4, (3 * K) // 7] = 65504.0
    r[5, K - 1] = -65504.0
    r = r.half()
    sub = torch.randint(-1023, 1024, (K,), generator=g).to(torch.float32) * 2.0 ** -24
    r[6] = sub.half()
    r[6, 0] = 2.0 ** -24
    r[7, ::3] = 0.0
    r[7, 1::6] = -0.0
    return r


def fake_quant_parts(x: torch.Tensor, w: torch.Tensor):
    """(decoded activation rows, activation scales, decoded weight rows, weight scales) of one linear, all on the host"""
    xq, xs = q_rows(x)
    wq, ws = q_rows(w)
    return decode(xq), xs, decode(wq), ws


def fake_quant_linear(x: torch.Tensor, w: torch.Tensor, bias=None) -> torch.Tensor:
    xd, xs, wd, ws = fake_quant_parts(x, w)
    y = (xd @ wd.t()) * xs[:, None] * ws[None, :]
    return y if bias is None else y + bias.float()


class FakeQuantLinear(nn.Module):
    def __init__(self, lin: nn.Linear):
        super().__init__()
        wq, ws = q_rows(lin.weight.detach())
        self.register_buffer("wd", decode(wq))
        self.register_buffer("ws", ws)
        self.bias = None if lin.bias is None else nn.Parameter(lin.bias.detach().clone().float())

    def forward(self, x):
        rows = x.reshape(-1, x.shape[-1])
        xq, xs = q_rows(rows)
        y = (decode(xq) @ self.wd.t()) * xs[:, None] * self.ws[None, :]
        if self.bias is not None:
            y = y + self.bias
        return y.reshape(*x.shape[:-1], -1)


def twin(model: nn.Module) -> nn.Module:
    """deep copy of an fp32 oracle DiT with the six linears of every block fake-quantised; the original is left as it is"""
    t = copy.deepcopy(model)
    for blk in t.transformer_blocks:
        for path in BLOCK_LINEARS:
            parent = blk
            *head, leaf = path.split(".")
            for name in head:
                parent = parent[int(name)] if name.isdigit() else getattr(parent, name)
            lin = parent[int(leaf)] if leaf.isdigit() else getattr(parent, leaf)
            assert isinstance(lin, nn.Linear), path
            if leaf.isdigit():
                parent[int(leaf)] = FakeQuantLinear(lin)
            else:
                setattr(parent, leaf, FakeQuantLinear(lin))
    return t


def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm()).item()

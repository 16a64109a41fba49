"""Host side of the CogVideoX DPM-Solver++ path without a GPU: the two entry points' refusals; ``CogVideoXDPMScheduler.coefficients``
against tests/dpm_oracle.py and the known answers of the infinite cases; its ``step`` on CPU tensors against the fp64 oracle and its generator draws; ``scheduler_from_config``; the
refusals of ``denoise`` and ``DistDiTDenoiser``."""
import json
import math

import pytest
import torch

import dpm_oracle as do
from c_interface import ALIGN, NULL, SHAPE, Host, entry
from cogvideox_support import tiny_cpu_model

STEPS = (4, 6, 50)


# ------------------------------------------------------------------------------------------------------------ the C interface
def _step_caller(h, temporal):
    common = dict(noise_rows=h.p, latents=h.p, latents_is_f32=1, x0_state=h.p, eps=h.p, B=1, F=4, C=16, H=8, W=12, p=2, cfg=2, order=2,
                  guidance=3.0, sqrt_alpha=0.8, sqrt_beta=0.6, m1=0.5, m2=-0.35, m3=1.4, m4=0.4, mn=0.7)
    if temporal:
        return entry("lkgd_dit_cfg_dpm_step_t", ldn=128, p_t=2, **common)
    return entry("lkgd_dit_cfg_dpm_step", ldn=64, **common)


@pytest.mark.parametrize("temporal", [False, True])
def test_dit_dpm_refusals(temporal):
    """one case per refusal of include/lkgd_hip_dit_dpm.h; host memory stands in for device pointers: a refused call never
    launches, so nothing dereferences them"""
    h = Host()
    step = _step_caller(h, temporal)
    width = 128 if temporal else 64
    # LKGD_E_NULL
    assert step(noise_rows=None) == NULL and step(latents=None) == NULL and step(x0_state=None) == NULL
    assert step(eps=None) == NULL                                  # mn != 0 needs the noise
    assert step(eps=None, mn=float("nan")) == NULL                 # NaN is not 0
    assert step(eps=None, mn=0.0, latents=None) == NULL
    # LKGD_E_SHAPE: what dit_shape_ok refuses - p = 1, 4, odd W, odd H, empty, C * 4 % 8, short ld, ld % 8
    for kw in (dict(p=1), dict(p=4), dict(W=13), dict(H=7), dict(B=0), dict(F=0), dict(C=0), dict(C=3), dict(ldn=width - 8),
               dict(ldn=width + 4)):
        assert step(**kw) == SHAPE, kw
    if temporal:
        for kw in (dict(p_t=1), dict(p_t=0), dict(p_t=4), dict(p_t=3, F=3), dict(F=3), dict(F=5)):      # p_t != 2, F % p_t
            assert step(**kw) == SHAPE, kw
    for kw in (dict(cfg=0), dict(cfg=3), dict(order=0), dict(order=3)):
        assert step(**kw) == SHAPE, kw
    # LKGD_E_ALIGN: rows not 16 bytes, x0_state not 4 bytes aligned
    assert step(noise_rows=h.p + 2) == ALIGN and step(noise_rows=h.p + 8) == ALIGN
    assert step(x0_state=h.p + 2) == ALIGN and step(x0_state=h.p + 1) == ALIGN
    # the order of the checks: NULL, then SHAPE, then ALIGN
    assert step(x0_state=None, cfg=3, noise_rows=None) == NULL and step(cfg=3, noise_rows=h.p + 2) == SHAPE


# ------------------------------------------------------------------------------------------------------------- coefficients
def _sched(steps, cls=None):
    from lkgd_amd import cogvideox as pc
    s = (cls or pc.CogVideoXDPMScheduler)()
    s.set_timesteps(steps)
    return s


def _loop_coefficients(s):
    out, t_back = [], None
    for t in s.timesteps.tolist():
        out.append((t, t_back, s.coefficients(t, t_back)))
        t_back = t
    return out


def test_the_tables_are_the_ddim_class_own():
    from lkgd_amd import cogvideox as pc
    d, m = _sched(6, pc.CogVideoXDDIMScheduler), _sched(6)
    assert torch.equal(d.alphas_cumprod, m.alphas_cumprod) and m.alphas_cumprod.dtype == torch.float64
    assert torch.equal(d.timesteps, m.timesteps) and float(m.final_alpha_cumprod) == 1.0
    assert type(m).coefficients is not type(d).coefficients and type(m).set_timesteps is type(d).set_timesteps      # shared, not copied
    assert m.order == 1 and m.init_noise_sigma == 1.0 and m.config._class_name == "CogVideoXDPMScheduler"
    for k in ("num_train_timesteps", "prediction_type", "timestep_spacing", "snr_shift_scale"):
        assert getattr(m.config, k) == getattr(d.config, k), k
    x = torch.randn(3)
    assert m.scale_model_input(x, 5) is x


@pytest.mark.parametrize("steps", STEPS)
def test_coefficients_vs_oracle(steps):
    """fp64 against fp64 (Python's libm against torch's): 1e-12 relative; everything finite; the tuple's names"""
    s = _sched(steps)
    ac = s.alphas_cumprod.tolist()
    assert ac[999] == 0.0                                             # zero terminal SNR: the lam = -inf case is real
    for t, t_back, k in _loop_coefficients(s):
        ref = do.coefficients(ac, t, t_back, steps)
        assert k._fields == ref._fields == ("sqrt_alpha", "sqrt_beta", "m1", "m2", "m3", "m4", "mn", "order")
        assert k.order == ref.order and isinstance(k.order, int)
        for name, a, b in zip(k._fields[:7], k[:7], ref[:7]):
            assert isinstance(a, float) and math.isfinite(a), (steps, t, name, a)
            assert abs(a - b) <= 1e-12 * abs(b), (steps, t, name, a, b)


def test_coefficients_known_answers():
    for steps in STEPS:
        s = _sched(steps)
        co = _loop_coefficients(s)
        assert len(co) == steps
        t, t_back, k = co[0]                                          # at = 0: lam = -inf, h = +inf
        assert (t, t_back) == (999, None) and k.order == 1 and k.m1 == 0.0 and k.sqrt_alpha == 0.0 and k.sqrt_beta == 1.0
        assert (k.m3, k.m4) == (1.0, 0.0)
        t, t_back, k = co[1]                                          # r = inf
        assert t_back == 999 and k.order == 2 and k.m3 == 1.0 and k.m4 == 0.0
        for _, _, k in co[2:-1]:
            assert k.order == 2 and k.m3 > 1.0 and abs(k.m3 - k.m4 - 1.0) < 1e-12 and k.m1 > 0 and k.m2 < 0 and k.mn > 0
    assert abs(_loop_coefficients(_sched(4))[0][2].m2 - -0.104718) < 5e-7
    for steps in (4, 50):                                             # prev = -1: onto final_alpha_cumprod = 1, lam_next = +inf
        t, t_back, k = _loop_coefficients(_sched(steps))[-1]
        assert t - 1000 // steps == -1 and t_back is not None
        assert k.order == 1 and (k.m1, k.m2, k.mn) == (0.0, -1.0, 0.0)
    t, t_back, k = _loop_coefficients(_sched(6))[-1]                  # 1000 // 6 = 166: prev = 0
    assert (t, t_back) == (166, 332) and k.order == 2 and abs(k.m3 - 3.17736) < 5e-6 and k.mn > 0
    t, t_back, k = _loop_coefficients(_sched(50))[-2]                 # the last second-order step of 50
    assert (t, t_back) == (39, 59) and k.order == 2 and abs(k.m3 - 1.80536) < 5e-6
    k = _sched(6).coefficients(499, 666)                              # the GPU file's decoy coefficients
    assert k.order == 2 and abs(k.m3 - 1.43) < 5e-3 and abs(k.mn - 0.72) < 5e-3
    assert _sched(6).coefficients(499, None).order == 1              # no previous step: first order


# ------------------------------------------------------------------------------------------------------------- the host step
def _step_data(seed, shape=(1, 3, 16, 8, 12)):
    g = torch.Generator().manual_seed(seed)
    return (2 * torch.randn(shape, generator=g), torch.randn(shape, generator=g), torch.randn(shape, generator=g).half())


def test_last_step_returns_x0_bitwise():
    """mn = 0, order 1, (m1, m2) = (0, -1): x' = 0 x - (-1) x0"""
    for steps in (4, 50):
        s = _sched(steps)
        ts = s.timesteps.tolist()
        noise, old, sample = _step_data(steps)
        prev, x0 = s.step(noise, old, ts[-1], ts[-2], sample, generator=torch.Generator().manual_seed(1))
        assert prev.dtype == x0.dtype == torch.float32 and prev.shape == sample.shape
        assert torch.equal(prev, x0) and bool(torch.isfinite(prev).all())
        assert torch.equal(x0, s.coefficients(ts[-1]).sqrt_alpha * sample.float() - s.coefficients(ts[-1]).sqrt_beta * noise)


@pytest.mark.parametrize("steps", STEPS)
def test_step_vs_fp64_oracle(steps):
    """every step of the loop's schedule on random data.  Bound: k 2^-24 S, S = the sum of the absolute values of the terms x'
    expands into and k = 10, the rounded operations on the longest path (the term m2 m3 sqrt_beta n of a second-order step):
    sqrt_beta -> fp32, sqrt_beta n, the subtraction to x0, m3 -> fp32, m3 x0, the subtraction to d, m2 -> fp32, m2 d, the
    subtraction, the addition of the noise term.  x0: k = 3 (a coefficient -> fp32, its product, the subtraction)"""
    s = _sched(steps)
    u = 2.0 ** -24
    for i, (t, t_back, k) in enumerate(_loop_coefficients(s)):
        noise, old, sample = _step_data(100 * steps + i)
        gen = torch.Generator().manual_seed(i)
        twin = torch.Generator().manual_seed(i)
        prev, x0 = s.step(noise, None if t_back is None else old, t, t_back, sample, generator=gen)
        for _ in range(k.order):
            eps = torch.randn(sample.shape, generator=twin, dtype=sample.dtype)
        assert eps.dtype == torch.float16
        ref, ref0, S, S0 = do.step_fp64(noise, old, sample, eps, do.coefficients(s.alphas_cumprod.tolist(), t, t_back, steps))
        err, err0 = (prev.double() - ref).abs(), (x0.double() - ref0).abs()
        print(f"\n{steps} steps, t = {t}: max err / (u S) = {(err / (u * S)).max().item():.2f} (bound 10), "
              f"x0 {(err0 / (u * S0)).max().item():.2f} (bound 3)")
        assert bool((err <= 10 * u * S).all()) and bool((err0 <= 3 * u * S0).all()), (steps, t)
        if k.mn != 0.0:                                               # the noise is in the result
            assert (prev.double() - (ref - k.mn * eps.double())).abs().max() > 0.1 * k.mn


def test_generator_draws():
    """4 steps: 1 + 2 + 2 + 1 draws of the sample's shape in fp16, the second of a pair used"""
    s = _sched(4)
    gen, twin = torch.Generator().manual_seed(77), torch.Generator().manual_seed(77)
    noise, _, sample = _step_data(9)
    old = t_back = None
    orders = []
    for t in s.timesteps.tolist():
        orders.append(s.coefficients(t, t_back).order)
        prev, old = s.step(noise, old, t, t_back, sample, generator=gen)
        sample, t_back = prev.half(), t
    assert orders == [1, 2, 2, 1]
    for n in orders:
        for _ in range(n):
            torch.randn(sample.shape, generator=twin, dtype=torch.float16)
    assert torch.equal(gen.get_state(), twin.get_state())
    torch.randn(sample.shape, generator=twin, dtype=torch.float16)
    assert not torch.equal(gen.get_state(), twin.get_state())        # one draw more is visible


def test_eta_raises():
    from lkgd_amd._lib import LkgdHipError
    s = _sched(4)
    noise, _, sample = _step_data(1)
    with pytest.raises(LkgdHipError, match="not built"):
        s.step(noise, None, 999, None, sample, eta=1.0)
    with pytest.raises(LkgdHipError, match="not built"):
        s.step(noise, None, 999, None, sample, 0.5)
    s.step(noise, None, 999, None, sample, eta=0.0)


# ------------------------------------------------------------------------------------------------------ scheduler_from_config
def _config(name, **over):
    """the released scheduler_config.json of the CogVideoX checkpoints"""
    c = {"_class_name": name, "_diffusers_version": "0.30.0", "beta_end": 0.012, "beta_schedule": "scaled_linear", "beta_start": 0.00085,
         "clip_sample": False, "clip_sample_range": 1.0, "num_train_timesteps": 1000, "prediction_type": "v_prediction",
         "rescale_betas_zero_snr": True, "sample_max_value": 1.0, "set_alpha_to_one": True, "snr_shift_scale": 1.0, "steps_offset": 0,
         "timestep_spacing": "trailing", "trained_betas": None}
    c.update(over)
    return c


def test_scheduler_from_config_dispatches_by_class_name(tmp_path):
    from lkgd_amd import cogvideox as pc
    for cls in (pc.CogVideoXDDIMScheduler, pc.CogVideoXDPMScheduler):
        s = pc.scheduler_from_config(_config(cls.__name__))
        assert type(s) is cls and s.config.snr_shift_scale == 1.0 and s.config._class_name == cls.__name__
        ref = cls(snr_shift_scale=1.0)
        assert torch.equal(s.alphas_cumprod, ref.alphas_cumprod) and not torch.equal(s.alphas_cumprod, cls().alphas_cumprod)
        # through a checkpoint directory: <dir>/scheduler/scheduler_config.json
        d = tmp_path / cls.__name__
        (d / "scheduler").mkdir(parents=True)
        json.dump(_config(cls.__name__, snr_shift_scale=3.0), open(d / "scheduler" / "scheduler_config.json", "w"))
        for where in (str(d), d):
            r = pc.scheduler_from_config(where)
            assert type(r) is cls and torch.equal(r.alphas_cumprod, cls().alphas_cumprod)


def test_scheduler_from_config_refusals_name_the_key(tmp_path):
    from lkgd_amd import cogvideox as pc
    from lkgd_amd._lib import LkgdHipError
    cases = [("prediction_type", "epsilon"), ("timestep_spacing", "leading"), ("timestep_spacing", "linspace"),
             ("rescale_betas_zero_snr", False), ("set_alpha_to_one", False), ("beta_schedule", "linear"),
             ("_class_name", "DDIMScheduler"), ("_class_name", None)]
    for name in ("CogVideoXDDIMScheduler", "CogVideoXDPMScheduler"):
        for key, value in cases:
            with pytest.raises(LkgdHipError, match=key):
                pc.scheduler_from_config(_config(name, **{key: value}))
    # a key the file leaves out has the published constructor's default: three of them are values that are not built
    for key in ("prediction_type", "timestep_spacing", "rescale_betas_zero_snr"):
        c = _config("CogVideoXDPMScheduler")
        del c[key]
        with pytest.raises(LkgdHipError, match=key):
            pc.scheduler_from_config(c)
    (tmp_path / "scheduler").mkdir()
    json.dump(_config("CogVideoXDPMScheduler", prediction_type="sample"), open(tmp_path / "scheduler" / "scheduler_config.json", "w"))
    with pytest.raises(LkgdHipError, match="prediction_type"):
        pc.scheduler_from_config(str(tmp_path))
    (tmp_path / "empty" / "scheduler").mkdir(parents=True)
    with pytest.raises(OSError, match="scheduler_config.json"):         # loading.load_config's own error, as for the other configs
        pc.scheduler_from_config(str(tmp_path / "empty"))


# ----------------------------------------------------------------------------------------------------------------- the loops
def test_denoise_refuses_what_is_no_scheduler():
    """the loop no longer runs DDIM updates for anything that has ``coefficients``: before any tensor is touched"""
    from types import SimpleNamespace
    from lkgd_amd import cogvideox as pc
    from lkgd_amd._lib import LkgdHipError

    class LooksLikeOne:
        timesteps = torch.tensor([999, 499])
        config = SimpleNamespace(num_train_timesteps=1000)

        def set_timesteps(self, n):
            pass

        def coefficients(self, t):
            return 1.0, 0.0, 1.0, 0.0
    m = tiny_cpu_model()
    z = torch.zeros(1, 3, 16, 8, 12)
    for bad in (LooksLikeOne(), SimpleNamespace(), None):
        with pytest.raises(LkgdHipError, match=type(bad).__name__):
            pc.denoise(m, bad, z, z, torch.zeros(2, 16, 4096), torch.zeros(1, 1, 1000), torch.zeros(1, 1, 1000), 2)
    import inspect
    assert inspect.signature(pc.denoise).parameters["generator"].default is None


def test_denoise_picks_its_step_by_the_declared_kind():
    """``step_kind`` of the class is what ``denoise`` reads: the three schedulers declare theirs, and a class that declares none, or
    one that is not built, is refused with the message of a class that is no scheduler at all"""
    from lkgd_amd import cogvideox as pc
    from lkgd_amd import ddim_inversion as di
    from lkgd_amd._lib import LkgdHipError
    assert (pc.CogVideoXDDIMScheduler.step_kind, pc.CogVideoXDPMScheduler.step_kind, di.DDIMInverseScheduler.step_kind) \
        == ("ddim", "dpm", "ddim")
    assert not hasattr(pc._CogVideoXSchedule, "step_kind")

    class Euler(pc.CogVideoXDDIMScheduler):
        step_kind = "euler"
    m = tiny_cpu_model()
    z = torch.zeros(1, 3, 16, 8, 12)
    for bad in (Euler(), pc._CogVideoXSchedule()):
        with pytest.raises(LkgdHipError) as e:
            pc.denoise(m, bad, z, z, torch.zeros(2, 16, 4096), torch.zeros(1, 1, 1000), torch.zeros(1, 1, 1000), 2)
        assert str(e.value) == (f"denoise: scheduler is a {type(bad).__module__}.{type(bad).__qualname__}; the loop's step is built "
                                "for CogVideoXDDIMScheduler and CogVideoXDPMScheduler")


def test_default_loop_placement_is_the_identity(monkeypatch):
    """``denoise`` without ``_placement``: every rows / text / noise answer is its argument, no shard, no hook"""
    from lkgd_amd import cogvideox as pc
    calls = []
    monkeypatch.setattr(pc.ops, "dit_patch_rows", lambda *a, **kw: calls.append((a, kw)) or "rows")
    place = pc.LoopPlacement()
    assert place.shard is None and place.after_step is None
    t = torch.zeros(2, 16, 4096)
    assert place.text(t) is t and place.noise(t) is t
    lat, img, out = object(), object(), object()
    assert place.rows(0, lat, img, out, 2) == "rows" and place.rows(1, lat, None, None, 2, p_t=2) == "rows"
    assert calls == [((lat, img, 2), dict(out=out)), ((lat, None, 2), dict(out=None, p_t=2))]


def test_dist_dit_denoiser_refuses_the_dpm_scheduler():
    """no process group is needed: the refusal comes before ``torch.distributed`` is asked anything"""
    import torch.distributed as dist
    from lkgd_amd import cogvideox as pc
    from lkgd_amd._lib import LkgdHipError
    from lkgd_amd.dist_run import DistDiTDenoiser
    assert not dist.is_initialized()
    m = tiny_cpu_model()
    with pytest.raises(LkgdHipError) as e:
        DistDiTDenoiser(m, pc.CogVideoXDPMScheduler(), 2, 0, 3)
    msg = str(e.value)
    assert "identical noise on every rank" in msg and "sharded DPM sampling is not built" in msg and "CogVideoXDDIMScheduler" in msg
    with pytest.raises(LkgdHipError, match="not initialised"):        # the DDIM class gets as far as it did
        DistDiTDenoiser(m, pc.CogVideoXDDIMScheduler(), 2, 0, 3)

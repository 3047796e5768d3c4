"""VCX_SAMPLER=dpmpp2m on a GPU-less host: the coefficient function against the fp64 restatement of the solver (tests/dpmpp_ref.py),
where its steps are first order, what the solver buys on a Gaussian toy model whose probability-flow ODE has a closed-form solution,
and the sampler's host side - switch, refusals, the loop on a CPU stand-in of ops.dpmpp2m_step against the restatement's loop."""
import math

import numpy as np
import pytest
import torch

from oracle.weights import synth_input
from tests import cpu_kernels, dpmpp_ref as R
from tests.tiny_config import TINY_UNET, tiny_model_params
from tests.util import SCHEDULE_BUFFERS, load_synth, rel_l2
from viewcrafter_amd.lvdm.models import utils_diffusion as U


# ------------------------------------------------------------------------------------------------------ schedules as the samplers hold them
def _alphas_cumprod(zero_snr):
    betas = U.make_beta_schedule("linear", 1000, linear_start=0.00085, linear_end=0.012)
    if zero_snr:
        betas = U.rescale_zero_terminal_snr(betas)
    return np.cumprod(1.0 - betas, axis=0).astype(np.float32)                  # the model's fp32 buffer


def _scale_arr(base=0.7, turning=400):
    return np.concatenate((np.linspace(1.0, base, turning), np.full(1000, base))).astype(np.float32)


def sampler_tables(S, spacing, rescale, multicond=False, zero_snr=True):
    """(alphas, alphas_prev, scale | None, scale_prev | None) of DDIMSampler.make_schedule (ddim.py / ddim_multiplecond.py), fp32."""
    acp = _alphas_cumprod(zero_snr)
    ts = U.make_ddim_timesteps(spacing, S, 1000, verbose=False)
    alphas = acp[ts]
    alphas_prev = np.concatenate([acp[0:1], acp[ts[:-1]]])
    if not rescale:
        return alphas, alphas_prev, None, None
    arr = _scale_arr()
    scale = arr[ts]
    scale_prev = np.concatenate([scale[0:1] if multicond else arr[0:1], scale[:-1]])
    return alphas, alphas_prev, scale, scale_prev


CASES = [(S, spacing, rescale, multicond, zero_snr) for S in (5, 10, 20, 50) for spacing in ("uniform", "uniform_trailing")
         for rescale, multicond in ((False, False), (True, False), (True, True)) for zero_snr in (True, False)]


@pytest.mark.parametrize("S,spacing,rescale,multicond,zero_snr", CASES)
def test_coefficients_match_the_restated_solver_and_orders_are_first_exactly_where_defined(S, spacing, rescale, multicond, zero_snr):
    tab = sampler_tables(S, spacing, rescale, multicond, zero_snr)
    c_h, order = U.dpmpp2m_coefficients(*tab)
    t = R.tables(*tab)
    want = [R.history_coefficient(t, i) for i in range(S)]
    assert c_h.dtype == np.float64 and c_h.shape == (S,)
    for i in range(S):
        assert abs(c_h[i] - want[i]) <= 1e-12 * abs(want[i]), (i, c_h[i], want[i])
    # first order: the first step taken, the step behind a timestep of zero SNR (lambda = -inf), the last step; second elsewhere
    inf_first = float(tab[0][S - 1]) == 0.0
    assert inf_first == (zero_snr and spacing == "uniform_trailing")
    expect = [1 if (i == S - 1 or i == 0 or (inf_first and i == S - 2)) else 2 for i in range(S)]
    assert list(order) == expect == R.orders(t)
    assert all((c_h[i] == 0.0) == (order[i] == 1) for i in range(S)) and np.isfinite(c_h).all()
    assert all(c_h[i] > 0 for i in range(S) if order[i] == 2)


def test_coefficients_need_one_entry_per_index():
    with pytest.raises(ValueError, match="one entry per DDIM index"):
        U.dpmpp2m_coefficients(np.full(4, 0.5), np.full(3, 0.6))


# ------------------------------------------------------------------------------------------------------ Gaussian toy
SIGMA0 = 0.8


def _toy_error(S, spacing, rescale, solver):
    """x0 ~ N(0, 0.8^2): the optimal denoiser is linear, the probability-flow ODE keeps x_t / std(x_t) constant, so the exact
    solution is x_T std_0 / std_T.  The PRODUCT's form of the step (DDIM at eta 0 + c_h (D - D_last), coefficients from
    dpmpp2m_coefficients) in fp64; returns the relative error of the final value."""
    al, al_p, sc, sc_p = [None if v is None else np.asarray(v, dtype=np.float64) for v in sampler_tables(S, spacing, rescale)]
    sc = np.ones(S) if sc is None else sc
    sc_p = np.ones(S) if sc_p is None else sc_p
    c_h, order = U.dpmpp2m_coefficients(al, al_p, sc, sc_p)
    a, b, a_p, b_p = np.sqrt(al), np.sqrt(1 - al), np.sqrt(al_p), np.sqrt(1 - al_p)
    std = lambda A, b_: math.sqrt(A * A * SIGMA0 ** 2 + b_ * b_)
    x, d_last = 1.0, None
    for i in range(S - 1, -1, -1):
        A = sc[i] * a[i]
        D = A * SIGMA0 ** 2 / (A * A * SIGMA0 ** 2 + b[i] ** 2) * x              # E[x0 | x_t]
        x0 = sc[i] * D
        e_t = (x - a[i] * x0) / b[i]
        x_new = a_p[i] * (x0 * sc_p[i] / sc[i]) + b_p[i] * e_t
        if solver == "2m" and order[i] == 2:
            x_new += c_h[i] * (D - d_last)
        x, d_last = x_new, D
    exact = 1.0 * std(sc_p[0] * a_p[0], b_p[0]) / std(sc[S - 1] * a[S - 1], b[S - 1])
    return abs(x - exact) / abs(exact)


@pytest.mark.parametrize("rescale", [True, False])
def test_gaussian_toy_trailing_spacing_20_solver_steps_beat_50_ddim_steps(rescale):
    e2m20, e2m50, eddim50 = (_toy_error(20, "uniform_trailing", rescale, "2m"), _toy_error(50, "uniform_trailing", rescale, "2m"),
                             _toy_error(50, "uniform_trailing", rescale, "ddim"))
    print(f"toy, uniform_trailing, rescale {rescale}: 2M-20 {e2m20:.3e}  2M-50 {e2m50:.3e}  DDIM-50 {eddim50:.3e}  "
          f"DDIM-20 {_toy_error(20, 'uniform_trailing', rescale, 'ddim'):.3e}")
    assert e2m20 < eddim50
    assert e2m50 < 0.25 * eddim50


@pytest.mark.parametrize("rescale", [True, False])
@pytest.mark.parametrize("S", [20, 25, 50])
def test_gaussian_toy_uniform_spacing_solver_beats_ddim_at_equal_steps(S, rescale):
    e2m, eddim = _toy_error(S, "uniform", rescale, "2m"), _toy_error(S, "uniform", rescale, "ddim")
    print(f"toy, uniform, rescale {rescale}, S = {S}: 2M {e2m:.3e}  DDIM {eddim:.3e}")
    assert e2m < eddim


# ------------------------------------------------------------------------------------------------------ the sampler's host side
def _dpmpp2m_step_cpu(calls):
    """include/vcx.h vcx_dpmpp2m_step_f32 in plain PyTorch, in the kernel's own form: the DDIM step of tests/test_hostgraph_cpu.py
    at sigma = 0 plus c_h (D - d_last)."""
    def run(x, v_cond, v_uncond, d_last, coef, inv_s, c_h, ws=None, v_img=None, cfg_img=0.0, d_out=None):
        calls.append(dict(c_h=float(c_h), inv_s=float(inv_s), d_last=d_last is not None, coef=list(coef), cfg_img=cfg_img,
                          inputs=(x, v_cond, v_uncond, v_img, None if d_last is None else d_last.clone())))
        sa, s1, a_prev, sigma, ratio, cfg, resc, is_v = [float(c) for c in coef[:8]]
        assert sigma == 0.0 and (d_last is not None or c_h == 0.0)
        if v_uncond is None:
            v = v_cond
        elif v_img is None:
            v = v_uncond + cfg * (v_cond - v_uncond)
        else:
            v = v_uncond + cfg_img * (v_img - v_uncond) + cfg * (v_cond - v_img)
        if v_uncond is not None and resc > 0:
            dims = tuple(range(1, v.dim()))
            std_pos, std_cfg = v_cond.double().std(dim=dims, keepdim=True), v.double().std(dim=dims, keepdim=True)
            v = (resc * (v.double() * (std_pos / std_cfg)) + (1 - resc) * v.double()).float()
        if is_v:
            e_t, x0 = sa * v + s1 * x, sa * x - s1 * v
        else:
            e_t, x0 = v, (x - s1 * v) / sa
        d = x0 * inv_s
        pred_x0 = x0 * ratio
        x_prev = math.sqrt(a_prev) * pred_x0 + math.sqrt(max(1.0 - a_prev, 0.0)) * e_t
        if c_h != 0.0:
            x_prev = x_prev + c_h * (d - d_last)
        if d_out is not None:
            d = d_out.copy_(d)
        calls[-1]["outputs"] = (x_prev, pred_x0, d.clone())
        return x_prev, pred_x0, d
    return run


@pytest.fixture
def tiny(monkeypatch):
    """The tiny latent-diffusion model (zero terminal SNR, dynamic rescale, v-prediction) on the CPU stand-ins of the kernels."""
    from viewcrafter_amd.config import Config
    from viewcrafter_amd.utils.diffusion_utils import instantiate_from_config
    cpu_kernels.install(monkeypatch)
    params = Config.wrap(tiny_model_params("lvdm.modules.networks.openaimodel3d.UNetModel", "lvdm.models.autoencoder.AutoencoderKL"))
    m = instantiate_from_config(Config(target="lvdm.models.ddpm3d.VIPLatentDiffusion", params=params)).eval()
    load_synth(m, skip=SCHEDULE_BUFFERS)
    return m


B, T, H, W = 1, 2, 16, 16


def _conds():
    cd = TINY_UNET["context_dim"]
    cat = synth_input("dpm_cat", (B, 4, T, H, W), scale=0.8)
    ctx, uctx = synth_input("dpm_ctx", (B, 77 + 16 * T, cd)), synth_input("dpm_uctx", (B, 77 + 16 * T, cd))
    cond = {"c_crossattn": [ctx], "c_concat": [cat]}
    uc = {"c_crossattn": [uctx], "c_concat": [cat]}
    uc2 = {"c_crossattn": [torch.cat([uctx[:, :77], ctx[:, 77:]], 1)], "c_concat": [cat]}
    return cond, uc, uc2, synth_input("dpm_xT", (B, 4, T, H, W))


def _sample(sampler, S=6, eta=0.0, spacing="uniform_trailing", multicond=False, **extra):
    cond, uc, uc2, x_T = _conds()
    with torch.no_grad():
        return sampler.sample(S=S, conditioning=cond, batch_size=B, shape=[4, T, H, W], verbose=False, unconditional_guidance_scale=7.5,
                              unconditional_conditioning=uc, eta=eta, cfg_img=3.0 if multicond else None, fs=torch.tensor([10] * B),
                              timestep_spacing=spacing, guidance_rescale=0.7, x_T=x_T,
                              unconditional_conditioning_img_nonetext=uc2 if multicond else None, **extra)[0]


def _sampler(model, multicond):
    from viewcrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    from viewcrafter_amd.lvdm.models.samplers.ddim_multiplecond import DDIMSampler as DDIMSamplerMulti
    return (DDIMSamplerMulti if multicond else DDIMSampler)(model)


@pytest.mark.parametrize("multicond", [False, True])
def test_sampler_loop_on_a_cpu_stand_in_equals_the_restated_loop(tiny, monkeypatch, multicond):
    """S = 6, uniform_trailing on zero-SNR tables (the first timestep has lambda = -inf): the product's loop - host coefficients, history
    buffer, order sequence - against tests/dpmpp_ref.py's loop around the same denoiser."""
    from viewcrafter_amd import ops
    calls = []
    monkeypatch.setattr(ops, "dpmpp2m_step", _dpmpp2m_step_cpu(calls))
    monkeypatch.setattr(ops, "ddim_step", lambda *a, **k: pytest.fail("ddim_step under VCX_SAMPLER=dpmpp2m"))
    monkeypatch.setenv("VCX_SAMPLER", "dpmpp2m")
    s = _sampler(tiny, multicond)
    state = torch.random.get_rng_state()
    got = _sample(s, multicond=multicond)
    assert torch.equal(torch.random.get_rng_state(), state), "the solver draws no noise (x_T was given)"
    assert [1 if c["c_h"] == 0.0 else 2 for c in calls] == [1, 1, 2, 2, 2, 1]
    assert [c["d_last"] for c in calls] == [False, False, True, True, True, False]
    assert not any(torch.is_tensor(v) and v.shape == got.shape for v in vars(s).values()), "the history must not live on the sampler"
    # every call on its own inputs: what the host passed (coefficients, 1 / s, which history) gives the restated step.  fp32 stand-in
    # against fp64: ~12 operations on magnitudes <= 60 are ~4e-5, bound 1e-4 as for the kernel (tests/test_dpmpp2m_gpu.py)
    for n, c in enumerate(calls):
        want = R.step_from_coef(*c["inputs"], c["coef"], c["cfg_img"], c["inv_s"], c["c_h"])
        errs = [float((g.double() - w).abs().max()) for g, w in zip(c["outputs"], want)]
        print(f"call {n}: c_h {c['c_h']:.4f} 1/s {c['inv_s']:.4f} max-abs errors x_prev / pred_x0 / D {errs}")
        assert max(errs) < 1e-4, (n, errs)

    cond, uc, uc2, x_T = _conds()
    h = s._host
    ab = [(float(h["sqrt_acp"][int(t)]), float(h["sqrt_1m_acp"][int(t)])) for t in s.ddim_timesteps]
    fs = torch.tensor([10] * B)

    def denoise(x, i):
        ts = torch.full((B,), int(s.ddim_timesteps[i]), dtype=torch.long)
        kw = dict(fs=fs, unconditional_conditioning_img_nonetext=uc2 if multicond else None)
        if multicond:
            kw["cfg_img"] = 3.0
        with torch.no_grad():
            return s._model_outputs(x.float(), ts, cond, uc, 7.5, kw)[:3]
    want, taken = R.loop(denoise, x_T, h["a"], h["a_prev"], s.ddim_scale_arr.numpy(), s.ddim_scale_arr_prev.numpy(), ab=ab, cfg=7.5,
                         cfg_img=3.0, rescale=0.7, is_v=True)
    e = rel_l2(got, want)
    print(f"sampler loop on the CPU stand-in vs the restated loop (multicond {multicond}): rel-L2 {e:.3e}, orders {taken}")
    assert taken == [1, 1, 2, 2, 2, 1]
    # The two loops hold their state in fp32 and fp64, so the denoiser - fp16 operands - sees inputs one fp32 ulp apart, which round
    # to different fp16 values in some elements: its outputs differ at the fp16 noise floor, and CFG 7.5 amplifies that.  The project's
    # bound for exactly this - a short CFG-7.5 trajectory of this model against a higher-precision run of the same arithmetic - is
    # DDIM_TOL = 1.6e-2 of tests/test_model_gpu.py (stated tolerance 3e-2).  A loop without the history term is 0.27 away (below).
    assert e <= 1.6e-2
    if multicond:
        return
    ddim, _ = R.loop(denoise, x_T, h["a"], h["a_prev"], s.ddim_scale_arr.numpy(), s.ddim_scale_arr_prev.numpy(), ab=ab, cfg=7.5, cfg_img=3.0,
                     rescale=0.7, is_v=True, first_order=True)
    assert rel_l2(got, ddim) > 2 * 3e-2, "within twice the stated trajectory tolerance of DDIM: this test could not tell the two apart"


def test_switch_parsing(monkeypatch):
    from viewcrafter_amd.lvdm.models.samplers import ddim
    monkeypatch.delenv("VCX_SAMPLER", raising=False)
    assert ddim.sampler_choice() == "ddim"
    for value, want in (("", "ddim"), ("ddim", "ddim"), ("dpmpp2m", "dpmpp2m"), ("DPMPP2M", "dpmpp2m"), (" dpmpp2m ", "dpmpp2m")):
        monkeypatch.setenv("VCX_SAMPLER", value)
        assert ddim.sampler_choice() == want
    for value in ("dpm", "unipc", "1", "dpmpp2m_sde"):
        monkeypatch.setenv("VCX_SAMPLER", value)
        with pytest.raises(ValueError, match="VCX_SAMPLER"):
            ddim.sampler_choice()


def test_unknown_sampler_and_nonzero_eta_are_refused_before_any_denoiser_call(tiny, monkeypatch):
    from viewcrafter_amd import ops
    monkeypatch.setattr(tiny, "apply_model", lambda *a, **k: pytest.fail("denoiser called"))
    monkeypatch.setattr(ops, "dpmpp2m_step", lambda *a, **k: pytest.fail("step called"))
    s = _sampler(tiny, False)
    monkeypatch.setenv("VCX_SAMPLER", "dpmpp2m")
    for eta in (1.0, 0.5):
        with pytest.raises(ValueError) as ei:
            _sample(s, eta=eta)
        msg = str(ei.value)
        assert "VCX_SAMPLER=dpmpp2m" in msg and "eta" in msg and "--ddim_eta 0" in msg
    s.make_schedule(6, ddim_discretize="uniform_trailing", ddim_eta=1.0, verbose=False)          # ddim_sampling called directly
    with pytest.raises(ValueError, match="--ddim_eta 0"):
        s.ddim_sampling(None, (B, 4, T, H, W), x_T=torch.zeros(B, 4, T, H, W))
    monkeypatch.setenv("VCX_SAMPLER", "euler")
    with pytest.raises(ValueError, match="VCX_SAMPLER"):
        _sample(s)


def test_mask_and_original_steps_stay_refused_under_the_solver(tiny, monkeypatch):
    from viewcrafter_amd import ops
    monkeypatch.setattr(tiny, "apply_model", lambda *a, **k: pytest.fail("denoiser called"))
    monkeypatch.setattr(ops, "dpmpp2m_step", lambda *a, **k: pytest.fail("step called"))
    monkeypatch.setenv("VCX_SAMPLER", "dpmpp2m")
    s = _sampler(tiny, False)
    x = torch.zeros(B, 4, T, H, W)
    with pytest.raises(NotImplementedError, match="mask"):
        _sample(s, mask=torch.ones_like(x), x0=x)
    s.make_schedule(6, ddim_discretize="uniform_trailing", ddim_eta=0.0, verbose=False)
    with pytest.raises(NotImplementedError):
        s.ddim_sampling(None, x.shape, x_T=x, ddim_use_original_steps=True)
    with pytest.raises(NotImplementedError):
        s.ddim_sampling(None, x.shape, x_T=x, noise_dropout=0.1)


@pytest.mark.parametrize("value", [None, "ddim"])
def test_without_the_switch_the_solver_op_is_never_called(tiny, monkeypatch, value):
    from tests.test_hostgraph_cpu import _ddim_step_cpu
    from viewcrafter_amd import ops
    steps = []

    def ddim_step(*a, **k):
        steps.append(1)
        return _ddim_step_cpu(*a, **k)
    monkeypatch.setattr(ops, "ddim_step", ddim_step)
    monkeypatch.setattr(ops, "dpmpp2m_step", lambda *a, **k: pytest.fail("dpmpp2m_step without VCX_SAMPLER=dpmpp2m"))
    if value is None:
        monkeypatch.delenv("VCX_SAMPLER", raising=False)
    else:
        monkeypatch.setenv("VCX_SAMPLER", value)
    out = _sample(_sampler(tiny, False), S=3, eta=1.0)
    assert len(steps) == 3 and torch.isfinite(out).all()


def test_guidance_group_outputs_in_one_reused_buffer_leave_the_history_intact(tiny, monkeypatch):
    """VCX_GUIDANCE_PARALLEL: the outputs a group exchanges are views of ONE buffer that the next exchange overwrites.  The solver's
    history must not depend on them outliving the step: a group that reuses its buffer gives the bits of one that hands out fresh
    tensors, and the checksum of the latent is taken at the start and compared at the end as under DDIM."""
    from viewcrafter_amd import ops
    monkeypatch.setattr(ops, "dpmpp2m_step", _dpmpp2m_step_cpu([]))
    monkeypatch.setenv("VCX_SAMPLER", "dpmpp2m")
    cond, uc, uc2, x_T = _conds()
    real, last = tiny.apply_model, {}

    def spy(x, t, c, **kw):
        last.update(x=x, t=t, kw=kw)
        return real(x, t, c, **kw)
    monkeypatch.setattr(tiny, "apply_model", spy)

    class Group:
        size, position = 2, 0

        def __init__(self, reuse):
            self.reuse, self.buf, self.events = reuse, None, []

        def checksum(self, img):
            self.events.append("checksum")
            return float(img.double().sum())

        def check_equal(self, img, also=None):
            self.events.append("check_equal")

        def exchange(self, v):
            self.events.append("exchange")
            other = real(last["x"], last["t"], uc, **last["kw"])               # what the rank at position 1 sends
            if not self.reuse:
                return [v.clone(), other]
            if self.buf is None:
                self.buf = torch.empty((2,) + tuple(v.shape))
            self.buf[0].copy_(v)
            self.buf[1].copy_(other)
            return [self.buf[0], self.buf[1]]
    outs = {}
    for reuse in (False, True):
        s = _sampler(tiny, False)
        s.guidance_group = Group(reuse)
        outs[reuse] = _sample(s, S=4)
        assert s.guidance_group.events == ["checksum"] + ["exchange"] * 4 + ["check_equal"]
    assert torch.isfinite(outs[True]).all() and torch.equal(outs[True], outs[False])

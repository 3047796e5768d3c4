"""DDIM sampler (reference lvdm/models/samplers/ddim.py) driving the gfx950 kernels.

Same public surface (DDIMSampler(model), make_schedule, sample, ddim_sampling, p_sample_ddim, stochastic_encode) and the
same arithmetic; what changes is where it runs:
  * all per-step scalars (a_t, a_prev, sigma_t, sqrt(1-a_t), dynamic-rescale ratio) are Python floats prepared once
    in make_schedule — the reference reads 6 device scalars per step (ddim.py:253-266), each a host sync;
  * classifier-free guidance runs cond and uncond as ONE batched UNet forward (B -> 2B) when both conditionings are
    dicts of tensors, instead of two sequential forwards (ddim.py:223-224);
  * CFG combine + guidance rescale (two per-sample std reductions) + v->eps/x0 + dynamic rescale + the x_{t-1} update
    are one fused launch pair, vcx_ddim_step_f32 (ddim.py:228-279 is ~30 element-wise kernels).

VCX_SAMPLER=dpmpp2m (not in the reference; unset or `ddim` = the loop above, launch for launch): ddim_sampling walks the same
timesteps with the DPM-Solver++(2M) update - the eta = 0 DDIM step plus a second-order term on the previous step's data prediction,
one fused launch pair as well (vcx_dpmpp2m_step_f32; coefficients from utils_diffusion.dpmpp2m_coefficients).  The solver is
deterministic: it needs eta = 0 and draws NO per-step noise, so after sampling the generator is not in the state the DDIM loop
leaves it in (DDIM draws one Gaussian per step even at eta = 0, like the reference).  p_sample_ddim and decode() stay DDIM.

VCX_FEATURE_CACHE=N (not in the reference; unset, 0 or 1 = the loops above, launch for launch): only the steps at loop positions
i % N == 0 run the whole UNet, the others a shallow forward on top of the deep feature the last full step left behind
(viewcrafter_amd/feature_cache.py; VCX_FEATURE_CACHE_DEPTH).  Either sampler, decode() and the multi-condition sampler go through it; the
cache object is local to the call, and every denoiser evaluation of a step that runs on its own (the one-after-the-other guidance
route, a guidance group's rank) has its own slot.
"""
import os

import numpy as np
import torch

from .... import ops
from ....feature_cache import feature_cache_plan, from_env as feature_cache_from_env
from ....interleave import step_yield
from ...common import noise_like
from ..utils_diffusion import dpmpp2m_coefficients, make_ddim_sampling_parameters, make_ddim_timesteps

SAMPLERS = ("ddim", "dpmpp2m")


def sampler_choice():
    """VCX_SAMPLER, read when a sample() call starts: `ddim` (also unset / empty) or `dpmpp2m`; anything else is an error."""
    name = os.environ.get("VCX_SAMPLER", "").strip().lower() or "ddim"
    if name not in SAMPLERS:
        raise ValueError(f"VCX_SAMPLER={os.environ['VCX_SAMPLER']!r}: expected one of {', '.join(SAMPLERS)}")
    return name


def _refuse_eta(what):
    return ValueError(f"VCX_SAMPLER=dpmpp2m is a deterministic solver and cannot run with {what}: pass --ddim_eta 0 (eta=0.0), or unset "
                      f"VCX_SAMPLER for the DDIM sampler")


class DDIMSampler(object):
    def __init__(self, model, schedule="linear", **kwargs):
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule
        self.counter = 0
        self._cfg_cache = None          # p_sample_ddim is public (decode() and bench.py call it without ddim_sampling)
        # classifier-free guidance evaluates the denoiser on the SAME x / t / c_concat under several c_crossattn: the layers
        # ahead of the first cross-attention are computed once (UNetModel._forward, cfg_repeat) - bit-identical results: every route decision
        # of the host graph is made per video (tests/test_batch_invariance_gpu.py checks both routes against each other at full width)
        self.share_cfg_prefix = True
        # one video on several GPUs (VCX_GUIDANCE_PARALLEL, viewcrafter_amd/parallel.py): a parallel.GuidanceGroup - this rank then
        # evaluates ONLY the conditioning of its position and receives the others' outputs (_split_outputs); None = everything here
        self.guidance_group = None

    def register_buffer(self, name, attr):
        if isinstance(attr, torch.Tensor):
            attr = attr.to(self.model.device)
        setattr(self, name, attr)

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        """Reference ddim.py:24-59."""
        self.ddim_timesteps = make_ddim_timesteps(ddim_discr_method=ddim_discretize, num_ddim_timesteps=ddim_num_steps,
                                                  num_ddpm_timesteps=self.ddpm_num_timesteps, verbose=verbose)
        acp = self.model.alphas_cumprod.detach().float().cpu()
        assert acp.shape[0] == self.ddpm_num_timesteps, "alphas have to be defined for each timestep"
        if self.model.use_dynamic_rescale:
            scale_arr = self.model.scale_arr.detach().float().cpu()
            self.ddim_scale_arr = scale_arr[self.ddim_timesteps]
            self.ddim_scale_arr_prev = torch.cat([scale_arr[0:1], self.ddim_scale_arr[:-1]])
        sigmas, alphas, alphas_prev = make_ddim_sampling_parameters(alphacums=acp, ddim_timesteps=self.ddim_timesteps,
                                                                    eta=ddim_eta, verbose=verbose)
        f32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32)
        self.register_buffer("ddim_sigmas", f32(sigmas))
        self.register_buffer("ddim_alphas", f32(alphas))
        self.register_buffer("ddim_alphas_prev", f32(alphas_prev))
        self.register_buffer("ddim_sqrt_one_minus_alphas", f32(np.sqrt(1. - alphas)))
        # host copies of every scalar the loop needs (fp32-rounded like the reference's device tables)
        self._host = dict(
            sigma=np.asarray(sigmas, dtype=np.float32), a=np.asarray(alphas, dtype=np.float32),
            a_prev=np.asarray(alphas_prev, dtype=np.float32),
            sqrt_acp=self.model.sqrt_alphas_cumprod.detach().float().cpu().numpy(),
            sqrt_1m_acp=self.model.sqrt_one_minus_alphas_cumprod.detach().float().cpu().numpy(),
        )
        if self.model.use_dynamic_rescale:
            self._host["ratio"] = (self.ddim_scale_arr_prev / self.ddim_scale_arr).numpy()

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, schedule_verbose=False, x_T=None, log_every_t=100,
               unconditional_guidance_scale=1., unconditional_conditioning=None, precision=None, fs=None,
               timestep_spacing="uniform", guidance_rescale=0.0, noise_source=None, **kwargs):
        """Reference ddim.py:62-134.  `noise_source` (not in the reference; default None = unchanged): a callable (shape, device) ->
        Gaussian tensor that replaces the sampler's own draws of x_T (when x_T is not given) and of every step's noise - several clips in
        one loop draw each clip's rows from that clip's generator (viewcrafter_amd/clip_batch.py)."""
        if conditioning is not None:
            first = conditioning[list(conditioning.keys())[0]] if isinstance(conditioning, dict) else conditioning
            cbs = (first[0] if isinstance(first, (list, tuple)) else first).shape[0]
            if cbs != batch_size:
                print(f"Warning: Got {cbs} conditionings but batch-size is {batch_size}")
        if sampler_choice() == "dpmpp2m" and float(eta) != 0.0:
            raise _refuse_eta(f"eta = {eta} (ddim_eta)")
        self.make_schedule(ddim_num_steps=S, ddim_discretize=timestep_spacing, ddim_eta=eta, verbose=schedule_verbose)
        if len(shape) == 3:
            size = (batch_size, *shape)
        elif len(shape) == 4:
            size = (batch_size, *shape)
        else:
            raise ValueError(f"shape must be (C,H,W) or (C,T,H,W), got {shape}")
        return self.ddim_sampling(conditioning, size, callback=callback, img_callback=img_callback,
                                  quantize_denoised=quantize_x0, mask=mask, x0=x0, ddim_use_original_steps=False,
                                  noise_dropout=noise_dropout, temperature=temperature, score_corrector=score_corrector,
                                  corrector_kwargs=corrector_kwargs, x_T=x_T, log_every_t=log_every_t,
                                  unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning, verbose=verbose,
                                  precision=precision, fs=fs, guidance_rescale=guidance_rescale, noise_source=noise_source, **kwargs)

    @torch.no_grad()
    def ddim_sampling(self, cond, shape, x_T=None, ddim_use_original_steps=False, callback=None, timesteps=None,
                      quantize_denoised=False, mask=None, x0=None, img_callback=None, log_every_t=100, temperature=1.,
                      noise_dropout=0., score_corrector=None, corrector_kwargs=None, unconditional_guidance_scale=1.,
                      unconditional_conditioning=None, verbose=True, precision=None, fs=None, guidance_rescale=0.0,
                      noise_source=None, **kwargs):
        """Reference ddim.py:137-205 (`noise_source`: see sample())."""
        if ddim_use_original_steps or quantize_denoised or score_corrector is not None or noise_dropout > 0.:
            raise NotImplementedError("DDPM-step / quantised / score-corrected sampling is not on the ViewCrafter path")
        device = self.model.betas.device
        b = shape[0]
        if x_T is not None:
            img = x_T.to(device=device, dtype=torch.float32)
        else:
            img = torch.randn(shape, device=device) if noise_source is None else noise_source(shape, device)
        if timesteps is None:
            timesteps = self.ddim_timesteps
        else:
            subset_end = int(min(timesteps / self.ddim_timesteps.shape[0], 1) * self.ddim_timesteps.shape[0]) - 1
            timesteps = self.ddim_timesteps[:subset_end]
        intermediates = {"x_inter": [img], "pred_x0": [img]}
        start_sum = None if self.guidance_group is None else self.guidance_group.checksum(img)      # compared with the final latent's
        time_range = np.flip(timesteps)
        total_steps = timesteps.shape[0]
        clean_cond = kwargs.pop("clean_cond", False)
        self._cfg_cache = None
        fcache, fplan = self._feature_cache(total_steps)
        if fcache is not None:
            kwargs = dict(kwargs, feature_cache=fcache)       # a keyword of the denoiser, like fs: p_sample_ddim and the solver's plan pass it on
        dpm = self._dpmpp2m_plan(mask, x0, kwargs) if sampler_choice() == "dpmpp2m" else None
        for i, step in enumerate(time_range):
            index = total_steps - i - 1
            if fcache is not None:
                fcache.set_mode("full" if fplan[i] else "shallow")
            ts = torch.full((b,), int(step), device=device, dtype=torch.long)
            if mask is not None:   # vestigial in ViewCrafter (mask is always None)
                assert x0 is not None
                img_orig = x0 if clean_cond else self.model.q_sample(x0, ts)
                img = img_orig * mask + (1. - mask) * img
            if dpm is not None:
                img, pred_x0 = self._dpmpp2m_step(dpm, img, cond, ts, index, first=i == 0,
                                                  unconditional_guidance_scale=unconditional_guidance_scale,
                                                  unconditional_conditioning=unconditional_conditioning, fs=fs,
                                                  guidance_rescale=guidance_rescale)
            else:
                img, pred_x0 = self.p_sample_ddim(img, cond, ts, index=index, temperature=temperature,
                                                  unconditional_guidance_scale=unconditional_guidance_scale,
                                                  unconditional_conditioning=unconditional_conditioning, mask=mask, x0=x0,
                                                  fs=fs, guidance_rescale=guidance_rescale, noise_source=noise_source, **kwargs)
            if callback:
                callback(i)
            if img_callback:
                img_callback(pred_x0, i)
            if self.guidance_group is not None and hasattr(self.guidance_group, "stats"):
                self.guidance_group.stats["steps"] += 1
            step_yield()           # two clips per GPU (viewcrafter_amd/interleave.py): the other clip's step is queued next; a no-op otherwise
            if index % log_every_t == 0 or index == total_steps - 1:
                intermediates["x_inter"].append(img)
                intermediates["pred_x0"].append(pred_x0)
        if self.guidance_group is not None:      # x was never sent inside the group: check once per video that it did stay bit-equal
            self.guidance_group.check_equal(img, also={"x_T": start_sum})
        return img, intermediates

    # ------------------------------------------------------------------ feature cache (VCX_FEATURE_CACHE)
    def _feature_cache(self, total_steps):
        """(cache object of this call, [step i is full]) or (None, None) with the switch off - read now, as VCX_SAMPLER is."""
        unet = getattr(getattr(self.model, "model", None), "diffusion_model", None)
        fcache, interval = feature_cache_from_env(unet)
        if fcache is None:
            return None, None
        return fcache, feature_cache_plan(total_steps, interval)

    def _evaluate(self, x, t, c, kwargs, position=0):
        """One denoiser evaluation; `position` = which of a step's evaluations it is where they run one after the other: each is a
        stream of its own from step to step, so each has its own slot of the feature cache."""
        fcache = kwargs.get("feature_cache")
        if fcache is not None:
            fcache.position = position
        return self.model.apply_model(x, t, c, **kwargs)

    # ------------------------------------------------------------------ DPM-Solver++(2M) (VCX_SAMPLER=dpmpp2m)
    def _dpmpp2m_plan(self, mask, x0, kwargs):
        """What one ddim_sampling call under the solver needs: per-index (c_h, order) and 1 / s from this sampler's own tables (the
        multi-condition sampler's scale_arr_prev differs), the keyword arguments of the denoiser, and the history slot.  The history
        lives in this dict, local to the call - not on self: two clips may interleave on samplers of one class, and the outputs a
        guidance group exchanges are views that the next exchange overwrites."""
        h = self._host
        if np.any(h["sigma"] != 0):
            raise _refuse_eta("a schedule made with eta != 0 (sigma_t != 0)")
        if mask is not None or x0 is not None:
            raise NotImplementedError("VCX_SAMPLER=dpmpp2m: mask / x0 blending is not implemented for the multistep solver")
        kw = dict(kwargs)
        if kw.pop("use_original_steps", False):
            raise NotImplementedError("not on the ViewCrafter path")
        for named in ("repeat_noise", "uc_type", "conditional_guidance_scale_temporal"):     # named parameters of p_sample_ddim: never the UNet's
            kw.pop(named, None)
        rescale = self.model.use_dynamic_rescale
        scale = self.ddim_scale_arr.numpy() if rescale else None
        c_h, order = dpmpp2m_coefficients(h["a"], h["a_prev"], scale, self.ddim_scale_arr_prev.numpy() if rescale else None)
        inv_s = 1.0 / scale.astype(np.float64) if rescale else np.ones(len(c_h))
        return dict(c_h=c_h, order=order, inv_s=inv_s, kwargs=kw, d=None)

    def _dpmpp2m_step(self, dpm, x, c, t, index, first, unconditional_guidance_scale, unconditional_conditioning, fs, guidance_rescale):
        """One solver step: the denoiser evaluations of p_sample_ddim, unchanged, then vcx_dpmpp2m_step_f32.  No noise is drawn."""
        x = x.float().contiguous()
        v_c, v_u, v_i, cfg_img = self._model_outputs(x, t, c, unconditional_conditioning, unconditional_guidance_scale,
                                                     dict(dpm["kwargs"], fs=fs))
        coef = self._step_coef(index, unconditional_guidance_scale, guidance_rescale, guided=v_u is not None, sigma=0.0)
        second = not first and dpm["order"][index] == 2           # the first step TAKEN has no history, whatever its index
        # D is written over the history it was computed from (a thread reads its element before it writes it): one buffer per call
        x_prev, pred_x0, dpm["d"] = ops.dpmpp2m_step(x, v_c.contiguous(), v_u.contiguous() if v_u is not None else None,
                                                     dpm["d"] if second else None, coef, float(dpm["inv_s"][index]),
                                                     float(dpm["c_h"][index]) if second else 0.0,
                                                     v_img=v_i.contiguous() if v_i is not None else None, cfg_img=cfg_img, d_out=dpm["d"])
        return x_prev, pred_x0

    def _step_coef(self, index, unconditional_guidance_scale, guidance_rescale, guided, sigma):
        """coef_host[0..8) of the step kernels (include/vcx.h) at DDIM index `index`."""
        h = self._host
        step_t = int(self.ddim_timesteps[index])   # == t[i] for all i, by construction of ddim_sampling
        coef = [float(h["sqrt_acp"][step_t]), float(h["sqrt_1m_acp"][step_t]), float(h["a_prev"][index]), sigma,
                float(h["ratio"][index]) if self.model.use_dynamic_rescale else 1.0, float(unconditional_guidance_scale),
                float(guidance_rescale) if guided else 0.0, 1.0 if self.model.parameterization == "v" else 0.0]
        if self.model.parameterization != "v":
            # eps-parameterisation reads the DDIM tables instead (ddim.py:259-260)
            coef[0], coef[1] = float(np.sqrt(h["a"][index])), float(np.sqrt(1. - h["a"][index]))
        return coef

    # ------------------------------------------------------------------ guidance evaluations split over the ranks of a group
    def _split_outputs(self, x, t, conds, kwargs):
        """One forward of batch b under conds[position] - no cfg_repeat, no stacking, whatever the conditionings' types - then one
        all_gather: every rank of the group returns the same len(conds) outputs, in the order of `conds`.  The exchange is outside the
        forward, so a captured forward (use_hip_graph) replays as it is."""
        group = self.guidance_group
        if group.size != len(conds):
            raise ValueError(f"the guidance group has {group.size} ranks, a step has {len(conds)} denoiser evaluations")
        stats = getattr(group, "stats", None)
        if stats is not None:
            stats["forwards"] += 1
            stats["batch"] = x.shape[0]
        # the outputs are views of the group's ONE reused buffer: valid until the next exchange (the step kernel reads them now)
        return group.exchange(self._evaluate(x, t, conds[group.position], kwargs, position=group.position))

    # ------------------------------------------------------------------ CFG batching
    @staticmethod
    def _batchable(c, *others):
        """True if all conditionings are dicts of equally shaped tensor lists, i.e. can be stacked on the batch axis."""
        if not isinstance(c, dict):
            return False
        for uc in others:
            if not isinstance(uc, dict) or set(c.keys()) != set(uc.keys()):
                return False
            for k in c:
                if not (isinstance(c[k], (list, tuple)) and isinstance(uc[k], (list, tuple)) and len(c[k]) == len(uc[k])):
                    return False
                if not all(torch.is_tensor(a) and torch.is_tensor(u) and a.shape == u.shape for a, u in zip(c[k], uc[k])):
                    return False
        return True

    def _shares_prefix(self, conds):
        """True if the conditionings differ only in c_crossattn (every other entry is the very same tensor object), the
        denoiser is the native UNet and the optimisation is enabled."""
        unet = getattr(getattr(self.model, "model", None), "diffusion_model", None)
        if not self.share_cfg_prefix or not hasattr(unet, "spatial_transformers"):
            return False
        return all(all(a is b_ for a, b_ in zip(conds[0][k], c[k])) for c in conds[1:] for k in c if k != "c_crossattn")

    def _cfg_cond(self, *conds, shared=False):
        """[cond ; uncond (; uncond_img)] stacked on the batch axis, built once per sample() call (so that the UNet's
        context-K/V cache, keyed on tensor identity, hits on every later step).  shared: only c_crossattn is stacked."""
        key = tuple(id(c) for c in conds) + (shared,)
        if self._cfg_cache is None or self._cfg_cache[0] != key:
            both = {k: (list(conds[0][k]) if (shared and k != "c_crossattn") else
                        [torch.cat(parts, dim=0) for parts in zip(*[c[k] for c in conds])]) for k in conds[0]}
            self._cfg_cache = (key, both, conds)
        return self._cfg_cache[1]

    def _apply_batched(self, x, t, conds, kwargs):
        """One UNet forward over len(conds) stacked conditionings; returns the per-conditioning outputs."""
        n, b = len(conds), x.shape[0]
        kw = dict(kwargs)
        if self._shares_prefix(conds):
            out = self._evaluate(x, t, self._cfg_cond(*conds, shared=True), dict(kw, cfg_repeat=n))
        else:
            if torch.is_tensor(kw.get("fs")):
                kw["fs"] = torch.cat([kw["fs"]] * n, 0)
            out = self._evaluate(torch.cat([x] * n, 0), torch.cat([t] * n, 0), self._cfg_cond(*conds), kw)
        return [out[i * b:(i + 1) * b] for i in range(n)]

    def _model_outputs(self, x, t, c, unconditional_conditioning, unconditional_guidance_scale, kwargs):
        """Denoiser evaluations of one step (reference ddim.py:218-231).  Returns (v_cond, v_uncond | None, v_img | None,
        cfg_img)."""
        if unconditional_conditioning is None or unconditional_guidance_scale == 1.:
            return self._evaluate(x, t, c, kwargs), None, None, 0.0
        if self.guidance_group is not None:
            v_c, v_u = self._split_outputs(x, t, (c, unconditional_conditioning), kwargs)
            return v_c, v_u, None, 0.0
        if self._batchable(c, unconditional_conditioning):
            v_c, v_u = self._apply_batched(x, t, (c, unconditional_conditioning), kwargs)
        elif isinstance(c, (torch.Tensor, dict)):
            v_c = self._evaluate(x, t, c, kwargs, position=0)
            v_u = self._evaluate(x, t, unconditional_conditioning, kwargs, position=1)
        else:
            raise NotImplementedError
        return v_c, v_u, None, 0.0

    @torch.no_grad()
    def p_sample_ddim(self, x, c, t, index, repeat_noise=False, use_original_steps=False, quantize_denoised=False,
                      temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1., unconditional_conditioning=None, uc_type=None,
                      conditional_guidance_scale_temporal=None, mask=None, x0=None, guidance_rescale=0.0, noise_source=None,
                      **kwargs):
        """Reference ddim.py:208-281 (`noise_source`: see sample())."""
        if use_original_steps or quantize_denoised or score_corrector is not None or noise_dropout > 0.:
            raise NotImplementedError("not on the ViewCrafter path")
        b, device = x.shape[0], x.device
        x = x.float().contiguous()
        v_c, v_u, v_i, cfg_img = self._model_outputs(x, t, c, unconditional_conditioning, unconditional_guidance_scale, kwargs)
        sigma = float(self._host["sigma"][index])
        coef = self._step_coef(index, unconditional_guidance_scale, guidance_rescale, guided=v_u is not None, sigma=sigma)
        # the reference draws the noise unconditionally (ddim.py:275), also when sigma_t = 0 (eta = 0): draw it too, so that a
        # fixed seed leaves the generator in the same state (the x_T of a following sample() call); the kernel skips it
        noise = noise_like(x.shape, device, repeat_noise) if noise_source is None else noise_source(x.shape, device)
        noise = noise * temperature if sigma != 0.0 else None
        x_prev, pred_x0 = ops.ddim_step(x, v_c.contiguous(), v_u.contiguous() if v_u is not None else None, noise, coef,
                                        v_img=v_i.contiguous() if v_i is not None else None, cfg_img=cfg_img)
        return x_prev, pred_x0

    @torch.no_grad()
    def decode(self, x_latent, cond, t_start, unconditional_guidance_scale=1.0, unconditional_conditioning=None,
               use_original_steps=False, callback=None):
        """Reference ddim.py:284-303: denoise `x_latent` (a latent noised to schedule index t_start, e.g. by stochastic_encode)
        through the first t_start DDIM steps.  Needs make_schedule() first, like the reference; extra sampler options
        (fs, guidance_rescale) are not part of this signature there either."""
        if use_original_steps:
            raise NotImplementedError("DDPM-step decoding is not on the ViewCrafter path")
        steps = np.asarray(self.ddim_timesteps)[:t_start]
        x = x_latent
        fcache, fplan = self._feature_cache(len(steps))
        fkw = {} if fcache is None else dict(feature_cache=fcache)
        for done, index in enumerate(range(len(steps) - 1, -1, -1)):
            ts = torch.full((x.shape[0],), int(steps[index]), device=x.device, dtype=torch.long)
            if fcache is not None:
                fcache.set_mode("full" if fplan[done] else "shallow")
            x, _ = self.p_sample_ddim(x, cond, ts, index=index, unconditional_guidance_scale=unconditional_guidance_scale,
                                      unconditional_conditioning=unconditional_conditioning, **fkw)
            if callback:
                callback(done)
        return x

    @torch.no_grad()
    def stochastic_encode(self, x0, t, use_original_steps=False, noise=None):
        """Reference ddim.py:306-319."""
        if use_original_steps:
            sa, s1 = self.model.sqrt_alphas_cumprod, self.model.sqrt_one_minus_alphas_cumprod
        else:
            sa, s1 = torch.sqrt(self.ddim_alphas), self.ddim_sqrt_one_minus_alphas
        if noise is None:
            noise = torch.randn_like(x0)
        shape = (x0.shape[0],) + (1,) * (x0.dim() - 1)
        return sa.gather(-1, t).reshape(shape) * x0 + s1.gather(-1, t).reshape(shape) * noise

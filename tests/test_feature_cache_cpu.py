"""The feature cache (VCX_FEATURE_CACHE, viewcrafter_amd/feature_cache.py) on a GPU-less machine: the schedule and the parsing of the two
variables, the host graph of a shallow forward on the CPU stand-ins of the kernels (tests/cpu_kernels.py, as tests/test_hostgraph_cpu.py
runs the plain forward) against the fp32 composition of tests/feature_cache_ref.py, slots and validity, and both samplers' loops.

Latent sizes.  The UNet halves the grid three times and doubles it again, so height and width are multiples of 8 and the pixel count of
level 0 is always a multiple of 64 (a 6 x 10 latent cannot pass the full forward, of the product or of the oracle: 3 x 5 -> 2 x 3 -> 4 x 6).
The kept target therefore carries moments and is read in place (split) at depths 0 .. 2; what a non-multiple would exercise - a COPIED
concat whose consumer makes its statistics pass - is what depth 3 keeps at both sizes here (level 1: 32 / 48 pixels per frame), and the
copied concat WITH moments is the VCX_CAT_SPLIT=0 case.  16 x 8 is one strip pair per frame, 8 x 24 an odd number of strips.
"""
import pytest
import torch

from oracle import lvdm_oracle as O
from oracle.weights import synth_input
from tests import cpu_kernels, dpmpp_ref, feature_cache_ref as R
from tests.tiny_config import TINY_UNET, tiny_model_params
from tests.util import SCHEDULE_BUFFERS, load_synth, rel_l2
from viewcrafter_amd import feature_cache as FC

# the bound tests/test_hostgraph_cpu.py has for the plain forward in this harness (same metric, same stand-in kernels, here on a subset of the layers)
UNET_TOL = 5e-3
# tests/test_model_gpu.py's bound for the uncached tiny CFG-7.5 trajectory against a higher-precision run of the same arithmetic
DDIM_TOL = 1.6e-2

SIZES = [(16, 8), (8, 24)]
CD = TINY_UNET["context_dim"]


# ------------------------------------------------------------------------------------------------------------- plan and parsing
@pytest.mark.parametrize("N", [2, 3, 5])
@pytest.mark.parametrize("steps", [1, 7, 50])
def test_plan_is_full_exactly_at_multiples_of_the_interval(N, steps):
    plan = FC.feature_cache_plan(steps, N)
    assert plan == [i % N == 0 for i in range(steps)] and len(plan) == steps and plan[0] is True
    assert sum(plan) == (steps + N - 1) // N


@pytest.mark.parametrize("value", [None, "", "0", "1", " 1 "])
def test_switch_is_off_for_unset_empty_zero_and_one(monkeypatch, value):
    monkeypatch.delenv("VCX_FEATURE_CACHE", raising=False)
    if value is not None:
        monkeypatch.setenv("VCX_FEATURE_CACHE", value)
    assert FC.feature_cache_interval() == 0 and FC.from_env() == (None, 0)
    assert FC.feature_cache_plan(5, FC.feature_cache_interval()) == [True] * 5


def test_switch_parsing(monkeypatch):
    monkeypatch.setenv("VCX_FEATURE_CACHE", "3")
    monkeypatch.delenv("VCX_FEATURE_CACHE_DEPTH", raising=False)
    fc, n = FC.from_env()
    assert n == 3 and fc.depth == 0 and fc.mode == "full" and fc.slot == (0, 0) and fc.filled == {}
    monkeypatch.setenv("VCX_FEATURE_CACHE_DEPTH", "2")
    assert FC.from_env()[0].depth == 2
    for bad in ("-1", "two", "2.5", "0x2"):
        monkeypatch.setenv("VCX_FEATURE_CACHE", bad)
        with pytest.raises(ValueError, match="VCX_FEATURE_CACHE="):
            FC.from_env()
    monkeypatch.setenv("VCX_FEATURE_CACHE", "2")
    for bad in ("-1", "deep", "11", "1.5"):
        monkeypatch.setenv("VCX_FEATURE_CACHE_DEPTH", bad)
        with pytest.raises(ValueError, match=r"VCX_FEATURE_CACHE_DEPTH=.*0 \.\. 10"):
            FC.feature_cache_depth(12)
    monkeypatch.setenv("VCX_FEATURE_CACHE_DEPTH", "10")
    assert FC.feature_cache_depth(12) == 10


# ------------------------------------------------------------------------------------------------------------- host graph
def _unet(monkeypatch, level, split=True):
    """tests/test_hostgraph_cpu.py::_unet, plus VCX_CAT_SPLIT."""
    cpu_kernels.install(monkeypatch)
    from viewcrafter_amd.lvdm.modules import attention, flow
    from viewcrafter_amd.lvdm.modules.networks import openaimodel3d as om
    for mod in (flow, attention, om):
        monkeypatch.setattr(mod, "GN_STATS_LEVEL", level, raising=False)
        monkeypatch.setattr(mod, "GN_EPILOGUE_STATS", level >= 1, raising=False)
        monkeypatch.setattr(mod, "CAT_SPLIT", split, raising=False)
    m = om.UNetModel(**TINY_UNET).eval()
    return m, load_synth(m)


def _inputs(tag, b, t, h, w, r=1, L=77 + 40):
    x = synth_input(f"fc_x_{tag}", (b, 8, t, h, w))
    ctx = synth_input(f"fc_ctx_{tag}", (b * r, L, CD))
    return x, torch.tensor([899, 419][:b]), ctx, torch.tensor([10, 3][:b])


_REFS = {}


def _reference(sd, size, depth):
    """(reference shallow output at the second inputs, computed once per size and depth)"""
    key = (size, depth)
    if key not in _REFS:
        h, w = size
        x0, t0, ctx, fs = _inputs(f"a{h}", 2, 3, h, w)
        x1, t1, _, _ = _inputs(f"b{h}", 2, 3, h, w)
        with torch.no_grad():
            y_full, kept = R.full_forward(sd, TINY_UNET, x0, t0, ctx, fs, depth)
            _REFS[key] = (y_full, R.shallow_forward(sd, TINY_UNET, x1, t1 - 40, ctx, fs, kept, depth))
    return _REFS[key]


def test_reference_shallow_forward_at_the_filling_inputs_is_the_oracles_forward():
    from viewcrafter_amd.lvdm.modules.networks.openaimodel3d import UNetModel
    sd = load_synth(UNetModel(**TINY_UNET))
    x, t, ctx, fs = _inputs("ref", 2, 3, 16, 8)
    with torch.no_grad():
        for depth in (0, 1, 2, 3, 10):
            y, kept = R.full_forward(sd, TINY_UNET, x, t, ctx, fs, depth)
            assert torch.equal(R.shallow_forward(sd, TINY_UNET, x, t, ctx, fs, kept, depth), y), depth
            assert torch.equal(y, O.unet_forward(sd, TINY_UNET, x, t, ctx, fs))


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("level,split", [(2, True), (2, False), (0, True)])
@pytest.mark.parametrize("depth", [0, 1, 2, 3])
def test_shallow_host_graph_vs_the_reference_composition(monkeypatch, depth, level, split, size):
    """Fill at (x0, t0), run shallow at another (x1, t1): against the fp32 composition; and shallow at the FILLING inputs gives the full
    forward's output bit for bit - the same skips are computed, and the kept tensor is exactly what the full forward fed to that block."""
    m, sd = _unet(monkeypatch, level, split)
    h, w = size
    x0, t0, ctx, fs = _inputs(f"a{h}", 2, 3, h, w)
    x1, t1, _, _ = _inputs(f"b{h}", 2, 3, h, w)
    fc = FC.FeatureCache(depth=depth)
    with torch.no_grad():
        plain = m(x0, t0, context=ctx, fs=fs)
        assert m._feature_store == {}
        y_full = m(x0, t0, context=ctx, fs=fs, feature_cache=fc)
        assert torch.equal(y_full, plain), "a full forward with a cache object is the plain forward"
        fc.set_mode("shallow")
        again = m(x0, t0, context=ctx, fs=fs, feature_cache=fc)
        y = m(x1, t1 - 40, context=ctx, fs=fs, feature_cache=fc)
        again2 = m(x0, t0, context=ctx, fs=fs, feature_cache=fc)
    assert torch.equal(again, y_full) and torch.equal(again2, y_full), "shallow at the filling inputs"
    ref_full, ref = _reference(sd, size, depth)
    e_full, e = rel_l2(y_full, ref_full), rel_l2(y, ref)
    store = next(iter(m._feature_store.values()))
    kind = "plain h" if level < 2 else f"target split={store['target'].split} moments={store['target'].moments is not None}"
    print(f"depth {depth} level {level} {h}x{w} ({kind}): full rel-L2 {e_full:.3e}, shallow rel-L2 vs the reference composition {e:.3e}; "
          f"shallow vs full output {rel_l2(y, y_full):.3e}")
    assert len(m._feature_store) == 1 and e <= UNET_TOL
    assert rel_l2(y, y_full) > 10 * UNET_TOL, "the second inputs must tell a shallow forward from a replay of the full one"
    if level == 2:          # depths 0 .. 2 keep a moment-carrying target, read in place unless VCX_CAT_SPLIT=0; depth 3 a copied concat without moments
        assert (store["target"].moments is not None) == (depth < 3) and store["target"].split == (split and depth < 3)


@pytest.mark.parametrize("r", [2, 3])
@pytest.mark.parametrize("depth", [0, 1])
def test_shallow_forward_under_the_shared_prefix_equals_the_replicated_batch(monkeypatch, depth, r):
    """cfg_repeat = r: one evaluation of the prefix, replicated where the conditionings enter - at depth 0 that is ahead of the output
    blocks (the input path stops in front of the first SpatialTransformer), at depth 1 inside input block 1.  Both forwards run the
    same launches per video on the stand-ins: bit-identical, rows of the replicated batch included."""
    m, _ = _unet(monkeypatch, 2)
    x0, t0, ctx, fs = _inputs("pa", 1, 3, 16, 8, r=r)
    x1, t1, _, _ = _inputs("pb", 1, 3, 16, 8)
    rep = lambda a: torch.cat([a] * r)
    shared, batch = FC.FeatureCache(depth=depth, lane=0), FC.FeatureCache(depth=depth, lane=1)
    with torch.no_grad():
        f1 = m(x0, t0, context=ctx, fs=fs, cfg_repeat=r, feature_cache=shared)
        f2 = m(rep(x0), rep(t0), context=ctx, fs=rep(fs), feature_cache=batch)
        shared.set_mode("shallow")
        batch.set_mode("shallow")
        y1 = m(x1, t1, context=ctx, fs=fs, cfg_repeat=r, feature_cache=shared)
        y2 = m(rep(x1), rep(t1), context=ctx, fs=rep(fs), feature_cache=batch)
    # the host BLAS behind the stand-ins is not batch-invariant (tests/test_hostgraph_cpu.py compares these two routes to rounding noise
    # for the same reason); on the GPU kernels this is bit for bit (tests/test_feature_cache_gpu.py)
    assert y1.shape == y2.shape == (r, 4, 3, 16, 8)
    assert rel_l2(f1, f2) <= UNET_TOL and rel_l2(y1, y2) <= UNET_TOL, (rel_l2(f1, f2), rel_l2(y1, y2))
    assert rel_l2(y1[0], y1[1]) > 1e-3, "the conditionings differ"


# ------------------------------------------------------------------------------------------------------------- slots and validity
def test_slots_and_validity(monkeypatch):
    m, _ = _unet(monkeypatch, 2)
    x0, t0, ctx, fs = _inputs("sa", 1, 3, 16, 8)
    x1, t1, ctx1, _ = _inputs("sb", 1, 3, 16, 8)
    xw = synth_input("fc_x_wide", (1, 8, 3, 16, 16))
    with torch.no_grad():
        m(x0, t0, context=ctx, fs=fs)
        assert m._feature_store == {} and m._graphs == {}, "no storage without the switch"
        fc = FC.FeatureCache(depth=1)
        fc.set_mode("shallow")
        with pytest.raises(RuntimeError, match="no full forward"):
            m(x0, t0, context=ctx, fs=fs, feature_cache=fc)
        fc.set_mode("full")
        ya = m(x0, t0, context=ctx, fs=fs, feature_cache=fc)
        fc.set_mode("shallow")
        with pytest.raises(RuntimeError, match="input shapes"):
            m(xw, t0, context=ctx, fs=fs, feature_cache=fc)
        with pytest.raises(RuntimeError, match="cfg_repeat"):
            m(x0, t0, context=torch.cat([ctx, ctx1]), fs=fs, cfg_repeat=2, feature_cache=fc)
        fc.position = 1
        with pytest.raises(RuntimeError, match="no full forward"):       # the neighbouring slot is empty
            m(x0, t0, context=ctx, fs=fs, feature_cache=fc)
        # a second sample() call's object does not inherit what the first left in the model's storage
        with pytest.raises(RuntimeError, match="no full forward"):
            other = FC.FeatureCache(depth=1)
            other.set_mode("shallow")
            m(x0, t0, context=ctx, fs=fs, feature_cache=other)
        # two slots, filled with different inputs, do not see each other
        fc.set_mode("full")
        yb = m(x1, t1, context=ctx1, fs=fs, feature_cache=fc)             # slot (0, 1)
        fc.set_mode("shallow")
        assert torch.equal(m(x1, t1, context=ctx1, fs=fs, feature_cache=fc), yb)
        fc.position = 0
        assert torch.equal(m(x0, t0, context=ctx, fs=fs, feature_cache=fc), ya)
        lane1 = FC.FeatureCache(depth=1, lane=1)
        m(x1, t1, context=ctx1, fs=fs, feature_cache=lane1)
        assert torch.equal(m(x0, t0, context=ctx, fs=fs, feature_cache=fc), ya), "another lane filled its own slot"
        assert len(m._feature_store) == 3
        with pytest.raises(NotImplementedError, match="features_adapter"):
            m(x0, t0, context=ctx, fs=fs, feature_cache=fc, features_adapter=[x0])
        with pytest.raises(ValueError, match=r"0 \.\. 10"):
            m(x0, t0, context=ctx, fs=fs, feature_cache=FC.FeatureCache(depth=11))
        m.drop_feature_cache()
        assert m._feature_store == {}
        with pytest.raises(RuntimeError, match="released"):
            m(x0, t0, context=ctx, fs=fs, feature_cache=fc)


def test_the_lane_of_an_interleaved_clip_is_part_of_its_slot():
    from viewcrafter_amd.interleave import current_lane, run_interleaved, step_yield
    assert current_lane() == 0

    def clip(item, index):
        lanes = []
        for _ in range(3):
            lanes.append(FC.FeatureCache().slot)
            step_yield()
        return lanes
    out = run_interleaved(clip, [(0, "a"), (1, "b"), (2, "c")], n_lanes=2)
    assert out == [[(0, 0)] * 3, [(1, 0)] * 3, [(0, 0)] * 3] and current_lane() == 0


# ------------------------------------------------------------------------------------------------------------- samplers
B, T, H, W = 1, 3, 16, 8


def _tiny(monkeypatch, zero_snr=True):
    """The tiny latent-diffusion model on the CPU stand-ins of the kernels (tests/test_dpmpp2m_cpu.py's fixture)."""
    from tests.test_dpmpp2m_cpu import _dpmpp2m_step_cpu
    from tests.test_hostgraph_cpu import _ddim_step_cpu
    from viewcrafter_amd import ops
    from viewcrafter_amd.config import Config
    from viewcrafter_amd.utils.diffusion_utils import instantiate_from_config
    cpu_kernels.install(monkeypatch)
    monkeypatch.setattr(ops, "ddim_step", _ddim_step_cpu)
    monkeypatch.setattr(ops, "dpmpp2m_step", _dpmpp2m_step_cpu([]))
    params = tiny_model_params("lvdm.modules.networks.openaimodel3d.UNetModel", "lvdm.models.autoencoder.AutoencoderKL")
    params["rescale_betas_zero_snr"] = zero_snr
    m = instantiate_from_config(Config(target="lvdm.models.ddpm3d.VIPLatentDiffusion", params=Config.wrap(params))).eval()
    load_synth(m, skip=SCHEDULE_BUFFERS)
    return m


@pytest.fixture
def tiny(monkeypatch):
    return _tiny(monkeypatch)


def _conds():
    cat = synth_input("fc_cat", (B, 4, T, H, W), scale=0.8)
    ctx, uctx = synth_input("fc_sctx", (B, 77 + 16 * T, CD)), synth_input("fc_suctx", (B, 77 + 16 * T, CD))
    return {"c_crossattn": [ctx], "c_concat": [cat]}, {"c_crossattn": [uctx], "c_concat": [cat]}, synth_input("fc_xT", (B, 4, T, H, W))


def _spy_modes(monkeypatch):
    modes = []
    set_mode = FC.FeatureCache.set_mode

    def spy(self, mode):
        modes.append(mode)
        return set_mode(self, mode)
    monkeypatch.setattr(FC.FeatureCache, "set_mode", spy)
    return modes


def _noise(tag):
    counter = [0]

    def draw(shape, *a, **k):
        counter[0] += 1
        return synth_input(f"fc_noise_{tag}_{counter[0]}", tuple(shape))
    return draw


def _oracle_denoiser(model, steps, N, depth, evals=2):
    cond, _, _ = _conds()
    sd = {k: v.float() for k, v in model.model.diffusion_model.state_dict().items()}
    prepare = lambda x, c: (torch.cat([x, cond["c_concat"][0]], 1), c)
    return R.CachedDenoiser(sd, TINY_UNET, torch.tensor([10] * B), steps, N, depth, evals, prepare)


@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("depth", [0, 2])
def test_ddim_loop_follows_the_plan_and_the_cached_oracle_trajectory(monkeypatch, eta, depth):
    """7 steps, N = 3, CFG 7.5: modes full, shallow, shallow, full, ...; final latent against oracle.ddim_sample around the stateful
    fp32 closure that follows the same plan.  eta = 1 runs on the tables WITHOUT the zero-terminal-SNR rescale: with it the first of 7
    trailing steps has sigma^2 = 1 - a_prev up to rounding, and the oracle (like the reference) takes the square root of
    1 - a_prev - sigma^2 = -6e-8 there - a NaN reference (at the 5 steps of tests/test_model_gpu.py the rounding falls the other way)."""
    import viewcrafter_amd.lvdm.models.samplers.ddim as ddim_mod
    zero_snr = eta == 0.0
    tiny = _tiny(monkeypatch, zero_snr)
    monkeypatch.setenv("VCX_FEATURE_CACHE", "3")
    monkeypatch.setenv("VCX_FEATURE_CACHE_DEPTH", str(depth))
    monkeypatch.setattr(ddim_mod, "noise_like", _noise("a"))
    modes = _spy_modes(monkeypatch)
    cond, uc, x_T = _conds()
    s = ddim_mod.DDIMSampler(tiny)
    with torch.no_grad():
        got, _ = s.sample(S=7, conditioning=cond, batch_size=B, shape=[4, T, H, W], verbose=False, unconditional_guidance_scale=7.5,
                          unconditional_conditioning=uc, eta=eta, fs=torch.tensor([10] * B), timestep_spacing="uniform_trailing",
                          guidance_rescale=0.7, x_T=x_T)
        plan = FC.feature_cache_plan(7, 3)
        assert modes == ["full" if p else "shallow" for p in plan] == ["full", "shallow", "shallow", "full", "shallow", "shallow", "full"]
        assert not any(isinstance(v, FC.FeatureCache) for v in vars(s).values()), "the cache object is local to the call"
        den = _oracle_denoiser(tiny, 7, 3, depth)
        want, _ = O.ddim_sample(den, O.diffusion_tables(zero_snr=zero_snr), O.dynamic_rescale_table(1000, 0.3, 400), x_T, cond["c_crossattn"][0],
                                uc["c_crossattn"][0], steps=7, eta=eta, cfg_scale=7.5, guidance_rescale=0.7, noise_fn=_noise("a"))
        assert den.modes == modes
        monkeypatch.delenv("VCX_FEATURE_CACHE")
        monkeypatch.setattr(ddim_mod, "noise_like", _noise("a"))
        plain, _ = s.sample(S=7, conditioning=cond, batch_size=B, shape=[4, T, H, W], verbose=False, unconditional_guidance_scale=7.5,
                            unconditional_conditioning=uc, eta=eta, fs=torch.tensor([10] * B), timestep_spacing="uniform_trailing",
                            guidance_rescale=0.7, x_T=x_T)
    e = rel_l2(got, want)
    print(f"cached DDIM trajectory (7 steps, N 3, depth {depth}, eta {eta}): rel-L2 vs the cached oracle {e:.3e}; the uncached trajectory is "
          f"{rel_l2(plain, want):.3e} away")
    assert torch.isfinite(want).all() and e <= DDIM_TOL
    assert len(modes) == 7, "the uncached run never touches a cache object"


def test_one_after_the_other_guidance_route_has_one_slot_per_evaluation(tiny, monkeypatch):
    """Conditionings that cannot be stacked (share_cfg_prefix off and a tensor-typed route is not available for dicts: the
    sampler's `_batchable` says no) run as two apply_model calls per step: positions 0 and 1, same latent as the batched route to the
    stand-ins' rounding noise."""
    import viewcrafter_amd.lvdm.models.samplers.ddim as ddim_mod
    monkeypatch.setenv("VCX_FEATURE_CACHE", "2")
    cond, uc, x_T = _conds()
    kw = dict(S=4, conditioning=cond, batch_size=B, shape=[4, T, H, W], verbose=False, unconditional_guidance_scale=7.5,
              unconditional_conditioning=uc, eta=0.0, fs=torch.tensor([10] * B), timestep_spacing="uniform_trailing", guidance_rescale=0.7, x_T=x_T)
    s = ddim_mod.DDIMSampler(tiny)
    seen = []
    apply_model = tiny.apply_model

    def spy(x, t, c, feature_cache=None, **k):
        seen.append((feature_cache.mode, feature_cache.slot, k.get("cfg_repeat", 1)))
        return apply_model(x, t, c, feature_cache=feature_cache, **k)
    monkeypatch.setattr(tiny, "apply_model", spy)
    with torch.no_grad():
        batched, _ = s.sample(**kw)
        n_batched = len(seen)
        monkeypatch.setattr(ddim_mod.DDIMSampler, "_batchable", staticmethod(lambda c, *o: False))
        serial, _ = s.sample(**kw)
    assert seen[:n_batched] == [("full", (0, 0), 2), ("shallow", (0, 0), 2)] * 2
    assert seen[n_batched:] == [("full", (0, 0), 1), ("full", (0, 1), 1), ("shallow", (0, 0), 1), ("shallow", (0, 1), 1)] * 2
    assert rel_l2(serial, batched) <= DDIM_TOL, rel_l2(serial, batched)


def test_dpmpp2m_loop_follows_the_plan_and_the_cached_restated_solver(tiny, monkeypatch):
    import viewcrafter_amd.lvdm.models.samplers.ddim as ddim_mod
    monkeypatch.setenv("VCX_FEATURE_CACHE", "3")
    monkeypatch.setenv("VCX_SAMPLER", "dpmpp2m")
    modes = _spy_modes(monkeypatch)
    cond, uc, x_T = _conds()
    s = ddim_mod.DDIMSampler(tiny)
    with torch.no_grad():
        got, _ = s.sample(S=7, conditioning=cond, batch_size=B, shape=[4, T, H, W], verbose=False, unconditional_guidance_scale=7.5,
                          unconditional_conditioning=uc, eta=0.0, fs=torch.tensor([10] * B), timestep_spacing="uniform_trailing",
                          guidance_rescale=0.7, x_T=x_T)
        assert modes == ["full", "shallow", "shallow", "full", "shallow", "shallow", "full"]
        den = _oracle_denoiser(tiny, 7, 3, 0)
        h = s._host
        ab = [(float(h["sqrt_acp"][int(t)]), float(h["sqrt_1m_acp"][int(t)])) for t in s.ddim_timesteps]

        def denoise(x, i):
            ts = torch.full((B,), int(s.ddim_timesteps[i]), dtype=torch.long)
            return den(x, ts, cond["c_crossattn"][0]), den(x, ts, uc["c_crossattn"][0]), None
        want, _ = dpmpp_ref.loop(denoise, x_T, h["a"], h["a_prev"], s.ddim_scale_arr.numpy(), s.ddim_scale_arr_prev.numpy(), ab=ab, cfg=7.5,
                                 rescale=0.7, is_v=True)
    e = rel_l2(got, want)
    print(f"cached DPM-Solver++(2M) trajectory (7 steps, N 3): rel-L2 vs the restated solver around the cached oracle {e:.3e}")
    assert den.modes == modes and e <= DDIM_TOL


def test_decode_goes_through_the_cache_as_ddim_sampling_does(tiny, monkeypatch):
    import viewcrafter_amd.lvdm.models.samplers.ddim as ddim_mod
    monkeypatch.setenv("VCX_FEATURE_CACHE", "2")
    modes = _spy_modes(monkeypatch)
    cond, uc, x_T = _conds()
    s = ddim_mod.DDIMSampler(tiny)
    with torch.no_grad():
        ref, _ = s.sample(S=4, conditioning=cond, batch_size=B, shape=[4, T, H, W], verbose=False, unconditional_guidance_scale=7.5,
                          unconditional_conditioning=uc, eta=0.0, timestep_spacing="uniform_trailing", x_T=x_T)
        out = s.decode(x_T.clone(), cond, t_start=4, unconditional_guidance_scale=7.5, unconditional_conditioning=uc)
    assert modes == ["full", "shallow"] * 4 and torch.equal(out, ref)

"""The feature cache (VCX_FEATURE_CACHE, viewcrafter_amd/feature_cache.py) on the MI355X: the tests of tests/test_feature_cache_cpu.py on the
real kernels (the latent sizes are explained there), bit-identity of what must not change (full forwards, the switch unset, batch rows,
the shared prefix, graph replay, two clips per GPU, batched clips, the one-after-the-other route, two guidance ranks)."""
import pytest
import torch

from oracle.weights import synth_input
from tests import feature_cache_ref as R
from tests.tiny_config import TINY_UNET, tiny_model_params
from tests.util import SCHEDULE_BUFFERS, load_synth, rel_l2
from viewcrafter_amd import feature_cache as FC

pytestmark = pytest.mark.gpu
DEV = "cuda"
CD = TINY_UNET["context_dim"]
# the bound tests/test_model_gpu.py has for the plain forward on the kernels against the fp32 oracle: the same metric and the same kernels,
# on a subset of the layers, on top of a kept feature that is itself the plain forward's (fp16) intermediate
UNET_TOL = 5e-3
SIZES = [(16, 8), (8, 24)]
MX = ("FF_MXFP8", "TATTN_MXFP8", "SATTN_MXFP8", "TCONV_MXFP8", "RESCONV_MXFP8")


def _new_unet():
    from viewcrafter_amd.lvdm.modules.networks.openaimodel3d import UNetModel
    m = UNetModel(**TINY_UNET).eval()
    sd = load_synth(m)
    return m.to(DEV), sd


@pytest.fixture(scope="module")
def unet():
    return _new_unet()


@pytest.fixture(scope="module")
def model():
    from viewcrafter_amd.config import Config
    from viewcrafter_amd.utils.diffusion_utils import instantiate_from_config
    params = Config.wrap(tiny_model_params("lvdm.modules.networks.openaimodel3d.UNetModel", "lvdm.models.autoencoder.AutoencoderKL"))
    m = instantiate_from_config(Config(target="lvdm.models.ddpm3d.VIPLatentDiffusion", params=params)).eval()
    load_synth(m, skip=SCHEDULE_BUFFERS)
    return m.to(DEV)


def _levels(monkeypatch, level, split=True):
    from viewcrafter_amd.lvdm.modules import attention, flow
    from viewcrafter_amd.lvdm.modules.networks import openaimodel3d as om
    for mod in (flow, attention, om):
        monkeypatch.setattr(mod, "GN_STATS_LEVEL", level, raising=False)
        monkeypatch.setattr(mod, "GN_EPILOGUE_STATS", level >= 1, raising=False)
        monkeypatch.setattr(mod, "CAT_SPLIT", split, raising=False)


def _inputs(tag, b, t, h, w, r=1, L=77 + 40):
    x = synth_input(f"fc_x_{tag}", (b, 8, t, h, w)).to(DEV)
    ctx = synth_input(f"fc_ctx_{tag}", (b * r, L, CD)).to(DEV)
    return x, torch.tensor([899, 419][:b], device=DEV), ctx, torch.tensor([10, 3][:b], device=DEV)


_REFS = {}


def _reference(sd, size, depth):
    """fp32 composition on the CPU, once per size and depth: (full output at the filling inputs, shallow output at the second inputs)"""
    key = (size, depth)
    if key not in _REFS:
        h, w = size
        x0, t0, ctx, fs = [a.cpu() for a in _inputs(f"a{h}", 2, 3, h, w)]
        x1, t1, _, _ = [a.cpu() for a in _inputs(f"b{h}", 2, 3, h, w)]
        with torch.no_grad():
            y_full, kept = R.full_forward(sd, TINY_UNET, x0, t0, ctx, fs, depth)
            _REFS[key] = (y_full, R.shallow_forward(sd, TINY_UNET, x1, t1 - 40, ctx, fs, kept, depth))
    return _REFS[key]


def _fill_and_go(m, size, depth):
    h, w = size
    x0, t0, ctx, fs = _inputs(f"a{h}", 2, 3, h, w)
    x1, t1, _, _ = _inputs(f"b{h}", 2, 3, h, w)
    fc = FC.FeatureCache(depth=depth)
    with torch.no_grad():
        plain = m(x0, t0, context=ctx, fs=fs).clone()
        assert m._feature_store == {}, "no storage without a cache object"
        y_full = m(x0, t0, context=ctx, fs=fs, feature_cache=fc).clone()
        fc.set_mode("shallow")
        again = m(x0, t0, context=ctx, fs=fs, feature_cache=fc).clone()
        y = m(x1, t1 - 40, context=ctx, fs=fs, feature_cache=fc).clone()
        again2 = m(x0, t0, context=ctx, fs=fs, feature_cache=fc).clone()
    torch.cuda.synchronize()
    assert torch.equal(y_full, plain), "a full forward with a cache object is the plain forward, bit for bit"
    assert torch.equal(again, y_full) and torch.equal(again2, y_full), "shallow at the filling inputs is the full forward's output, bit for bit"
    store = next(iter(m._feature_store.values()))
    m.drop_feature_cache()
    return y_full, y, store


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("level,split", [(2, True), (2, False), (0, True)])
@pytest.mark.parametrize("depth", [0, 1, 2, 3])
def test_shallow_forward_vs_the_reference_composition(unet, monkeypatch, depth, level, split, size):
    m, sd = unet
    _levels(monkeypatch, level, split)
    y_full, y, store = _fill_and_go(m, size, depth)
    ref_full, ref = _reference(sd, size, depth)
    e_full, e = rel_l2(y_full, ref_full), rel_l2(y, ref)
    kind = "plain h" if level < 2 else f"target split={store['target'].split} moments={store['target'].moments is not None}"
    print(f"depth {depth} level {level} {size} ({kind}): full rel-L2 {e_full:.3e}, shallow rel-L2 vs the reference composition {e:.3e}")
    assert torch.isfinite(y).all() and e <= UNET_TOL
    assert rel_l2(y, y_full) > 10 * UNET_TOL, "the second inputs must tell a shallow forward from a replay of the full one"
    if level == 2:          # depths 0 .. 2 keep a moment-carrying target, read in place unless VCX_CAT_SPLIT=0; depth 3 a copied concat without moments
        assert (store["target"].moments is not None) == (depth < 3) and store["target"].split == (split and depth < 3)


@pytest.mark.parametrize("depth", [0, 2])
def test_shallow_at_the_filling_inputs_with_all_five_mxfp8_switches(monkeypatch, depth):
    """Only the bit-equality half: the MX layers' accuracy has its own files."""
    from viewcrafter_amd.lvdm.modules import attention
    from viewcrafter_amd.lvdm.modules.networks import openaimodel3d as om
    for name in MX:
        mod = attention if hasattr(attention, name) else om
        monkeypatch.setattr(mod, name, True)
        monkeypatch.setattr(mod, name + "_SKIP_DIMS", frozenset())
    m, _ = _new_unet()
    y_full, y, _ = _fill_and_go(m, (16, 8), depth)
    assert torch.isfinite(y).all() and not torch.equal(y, y_full)


@pytest.mark.parametrize("r", [2, 3])
@pytest.mark.parametrize("depth", [0, 1])
def test_shallow_forward_under_the_shared_prefix_is_the_replicated_batch_bit_for_bit(unet, depth, r):
    """At depth 0 the replication takes the other branch (ahead of the output blocks: the input path stops in front of the first
    SpatialTransformer), at depth 1 it happens inside input block 1."""
    m, _ = unet
    x0, t0, ctx, fs = _inputs("pa", 1, 3, 16, 8, r=r)
    x1, t1, _, _ = _inputs("pb", 1, 3, 16, 8)
    rep = lambda a: torch.cat([a] * r)
    shared, batch = FC.FeatureCache(depth=depth, lane=0), FC.FeatureCache(depth=depth, lane=1)
    with torch.no_grad():
        f1 = m(x0, t0, context=ctx, fs=fs, cfg_repeat=r, feature_cache=shared).clone()
        f2 = m(rep(x0), rep(t0), context=ctx, fs=rep(fs), feature_cache=batch).clone()
        shared.set_mode("shallow")
        batch.set_mode("shallow")
        y1 = m(x1, t1, context=ctx, fs=fs, cfg_repeat=r, feature_cache=shared).clone()
        y2 = m(rep(x1), rep(t1), context=ctx, fs=rep(fs), feature_cache=batch).clone()
    m.drop_feature_cache()
    assert torch.equal(f1, f2) and torch.equal(y1, y2)
    assert not torch.equal(y1[0], y1[1]) and not torch.equal(y1, f1)


def test_rows_of_a_shallow_forward_do_not_depend_on_the_batch(unet):
    """tests/test_batch_invariance_gpu.py's contract on shallow forwards: row 0 of B = 2 is the B = 1 forward of the same video."""
    m, _ = unet
    for depth in (0, 2):
        x0, t0, ctx, fs = _inputs("ra", 2, 3, 16, 8)
        x1, t1, _, _ = _inputs("rb", 2, 3, 16, 8)
        two, ones = FC.FeatureCache(depth=depth, lane=0), [FC.FeatureCache(depth=depth, lane=1 + i) for i in range(2)]
        with torch.no_grad():
            m(x0, t0, context=ctx, fs=fs, feature_cache=two)
            for i, fc in enumerate(ones):
                m(x0[i:i + 1], t0[i:i + 1], context=ctx[i:i + 1].contiguous(), fs=fs[i:i + 1], feature_cache=fc)
                fc.set_mode("shallow")
            two.set_mode("shallow")
            y2 = m(x1, t1, context=ctx, fs=fs, feature_cache=two).clone()
            y1 = [m(x1[i:i + 1], t1[i:i + 1], context=ctx[i:i + 1].contiguous(), fs=fs[i:i + 1], feature_cache=fc).clone() for i, fc in enumerate(ones)]
        m.drop_feature_cache()
        for i in range(2):
            assert torch.equal(y2[i:i + 1], y1[i]), f"depth {depth}: row {i} of the B = 2 shallow forward differs from its B = 1 forward"


def test_graph_replay_of_full_and_shallow_forwards_is_bit_identical_to_eager(unet):
    """full, shallow, shallow, full, shallow with fresh inputs each time, two slots alive at once (the two evaluations of the
    one-after-the-other route): every graphed output equals the eager one; four graphs serve the ten calls; eager works afterwards."""
    m, _ = unet
    T, h, w = 3, 16, 8
    ctxs = [synth_input(f"fcg_ctx{p}", (1, 77 + 16 * T, CD)).to(DEV) for p in range(2)]
    fs = torch.tensor([10], device=DEV)
    seq = ["full", "shallow", "shallow", "full", "shallow"]

    def run(graphed):
        fc, outs = FC.FeatureCache(depth=1), []
        m.use_hip_graph = graphed
        try:
            for k, mode in enumerate(seq):
                x = synth_input(f"fcg_x{k}", (1, 8, T, h, w)).to(DEV)
                t = torch.full((1,), 999 - 150 * k, device=DEV, dtype=torch.long)
                fc.set_mode(mode)
                for pos in range(2):
                    fc.position = pos
                    with torch.no_grad():
                        outs.append(m(x, t, context=ctxs[pos], fs=fs, feature_cache=fc).clone())
        finally:
            m.use_hip_graph = False
        torch.cuda.synchronize()
        return outs
    eager = run(False)
    m.drop_feature_cache()
    graphed = run(True)
    assert len(m._graphs) == 4, f"{len(m._graphs)} graphs: one per (mode, slot) must serve all replays"
    assert len(m._feature_store) == 2
    for k, (a, b) in enumerate(zip(eager, graphed)):
        assert torch.equal(a, b), f"call {k} ({seq[k // 2]}, slot {k % 2}) differs between replay and eager"
    assert not torch.equal(eager[2], eager[4]) and not torch.equal(eager[0], eager[1])
    again = run(False)                          # eager on the storage the graphs address
    assert all(torch.equal(a, b) for a, b in zip(eager, again))
    fc = FC.FeatureCache(depth=1)
    fc.set_mode("shallow")
    m.use_hip_graph = True
    try:
        with pytest.raises(RuntimeError, match="no full forward"):
            m(synth_input("fcg_x0", (1, 8, T, h, w)).to(DEV), torch.tensor([5], device=DEV), context=ctxs[0], fs=fs, feature_cache=fc)
    finally:
        m.use_hip_graph = False
    m.drop_feature_cache()
    assert m._graphs == {} and m._feature_store == {}


# ------------------------------------------------------------------------------------------------------------- samplers
def _sample(model, b=1, steps=6, eta=0.0, **extra):
    from viewcrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    t, h, w = 3, 16, 8
    cat = synth_input("fcs_cat", (b, 4, t, h, w), scale=0.8).to(DEV)
    ctx, uctx = synth_input("fcs_ctx", (b, 77 + 16 * t, CD)).to(DEV), synth_input("fcs_uctx", (b, 77 + 16 * t, CD)).to(DEV)
    cond, uc = {"c_crossattn": [ctx], "c_concat": [cat]}, {"c_crossattn": [uctx], "c_concat": [cat]}
    x_T = synth_input("fcs_xT", (b, 4, t, h, w)).to(DEV)
    torch.manual_seed(77)
    with torch.no_grad():
        out, _ = DDIMSampler(model).sample(S=steps, conditioning=cond, batch_size=b, shape=[4, t, h, w], verbose=False,
                                           unconditional_guidance_scale=7.5, unconditional_conditioning=uc, eta=eta,
                                           fs=torch.tensor([10] * b, device=DEV), timestep_spacing="uniform_trailing", guidance_rescale=0.7,
                                           x_T=x_T, **extra)
    torch.cuda.synchronize()
    return out.clone()


def test_sampler_with_the_switch_unset_never_builds_a_cache(model, monkeypatch):
    """Unset, 0 and 1: the same latent bit for bit, no cache object reaches the denoiser, no storage on the UNet."""
    unet = model.model.diffusion_model
    seen = []
    apply_model = model.apply_model

    def spy(x, t, c, **k):
        seen.append("feature_cache" in k)
        return apply_model(x, t, c, **k)
    monkeypatch.setattr(model, "apply_model", spy)
    monkeypatch.delenv("VCX_FEATURE_CACHE", raising=False)
    want = _sample(model)
    for value in ("0", "1", ""):
        monkeypatch.setenv("VCX_FEATURE_CACHE", value)
        assert torch.equal(_sample(model), want)
    assert seen and not any(seen) and unet._feature_store == {}
    monkeypatch.setenv("VCX_FEATURE_CACHE", "2")
    cached = _sample(model)
    assert seen[-1] and torch.isfinite(cached).all() and not torch.equal(cached, want)
    unet.drop_feature_cache()


@pytest.mark.parametrize("b", [1, 2])
def test_one_after_the_other_guidance_route_gives_the_batched_routes_bits(model, monkeypatch, b):
    """Two apply_model calls per step, each in its own slot, against the stacked forward with the shared prefix (one slot): the bits
    tests/test_guidance_parallel_gpu.py promises for these two routes without the cache, eta 1 included."""
    import viewcrafter_amd.lvdm.models.samplers.ddim as ddim_mod
    monkeypatch.setenv("VCX_FEATURE_CACHE", "3")
    monkeypatch.setenv("VCX_FEATURE_CACHE_DEPTH", "1")
    batched = _sample(model, b=b, eta=1.0)
    monkeypatch.setattr(ddim_mod.DDIMSampler, "_batchable", staticmethod(lambda c, *o: False))
    serial = _sample(model, b=b, eta=1.0)
    assert len(model.model.diffusion_model._feature_store) == 3      # (0, 0) at cfg_repeat 2, (0, 0) and (0, 1) at cfg_repeat 1
    model.model.diffusion_model.drop_feature_cache()
    assert torch.equal(serial, batched), f"{int((serial != batched).sum())} elements differ"


def test_dpmpp2m_and_graphed_sampling_go_through_the_cache(model, monkeypatch):
    """VCX_SAMPLER=dpmpp2m with the cache, eager against graph replay of the same loop: bit-identical."""
    unet = model.model.diffusion_model
    monkeypatch.setenv("VCX_FEATURE_CACHE", "2")
    monkeypatch.setenv("VCX_SAMPLER", "dpmpp2m")
    eager = _sample(model)
    unet.drop_feature_cache()
    unet.use_hip_graph = True
    try:
        graphed = _sample(model)
        n_graphs = len(unet._graphs)
    finally:
        unet.use_hip_graph = False
        unet.drop_feature_cache()
    assert n_graphs == 2 and torch.equal(graphed, eager)


# ------------------------------------------------------------------------------------------------------------- clips
@pytest.fixture(scope="module")
def igs_model():
    """tests/test_clip_batch_gpu.py's model: the tiny hybrid model with the tiny OpenCLIP towers and Resampler."""
    from tests.tiny_config import CLIP_TINY, CLIP_TINY_CFG, igs_model_params
    from viewcrafter_amd.config import Config
    from viewcrafter_amd.lvdm.modules.encoders import condition as cond
    from viewcrafter_amd.utils.diffusion_utils import instantiate_from_config
    cond.CLIP_CONFIGS[CLIP_TINY] = CLIP_TINY_CFG
    E = "lvdm.modules.encoders."
    params = Config.wrap(igs_model_params("lvdm.modules.networks.openaimodel3d.UNetModel", "lvdm.models.autoencoder.AutoencoderKL",
                                          E + "condition.FrozenOpenCLIPEmbedder", E + "condition.FrozenOpenCLIPImageEmbedderV2",
                                          E + "resampler.Resampler"))
    m = instantiate_from_config(Config(target="lvdm.models.ddpm3d.VIPLatentDiffusion", params=params)).eval()
    load_synth(m, skip=SCHEDULE_BUFFERS)
    return m.to(DEV)


def _clips_solo_lanes_batched(model, clips, noise_shape, steps=4):
    """Every clip's video: alone (one after the other), two at a time on two streams (VCX_CLIPS_PER_GPU=2), two in one loop (VCX_CLIP_BATCH=2)."""
    from viewcrafter_amd import clip_batch, parallel
    from viewcrafter_amd.utils.diffusion_utils import image_guided_synthesis, image_guided_synthesis_clips
    kw = dict(n_samples=1, ddim_steps=steps, ddim_eta=1.0, unconditional_guidance_scale=7.5, cfg_img=None, fs=10, text_input=False,
              multiple_cond_cfg=False, timestep_spacing="uniform_trailing", guidance_rescale=0.7, condition_index=[0])

    def one(videos, index):
        torch.manual_seed(900 + index)
        with torch.no_grad():
            return image_guided_synthesis(model, [""], videos, noise_shape, **kw)

    def group(videos, indices):
        streams = clip_batch.ClipStreams([900 + i for i in indices])
        with torch.no_grad():
            outs = image_guided_synthesis_clips(model, [""], videos, noise_shape, streams=streams, **kw)
        streams.finish()
        return outs

    def done(res):
        torch.cuda.synchronize()
        return [res[i].clone() for i in range(len(clips))]
    solo = done(parallel.run_sharded(one, clips, gather=False, lanes=1))
    lanes = done(parallel.run_sharded(one, clips, gather=False, lanes=2))
    batched = done(parallel.run_sharded_batched(group, clips, 2, gather=False))
    return solo, lanes, batched


def test_two_clips_per_gpu_and_batched_clips_equal_each_clips_own_cached_run(igs_model, monkeypatch):
    """The lanes of VCX_CLIPS_PER_GPU=2 share the model, not a slot: each of two DIFFERENT clips is its own solo cached video bit for
    bit; VCX_CLIP_BATCH=2 is one slot of batch 2 with the same rows."""
    from tests.tiny_config import IGS_H, IGS_T, IGS_W
    monkeypatch.setenv("VCX_FEATURE_CACHE", "2")
    clips = [torch.tanh(synth_input(f"fc_clip{i}", (1, 3, IGS_T, IGS_H, IGS_W))).to(DEV) for i in range(2)]
    solo, lanes, batched = _clips_solo_lanes_batched(igs_model, clips, [1, 4, IGS_T, IGS_H // 8, IGS_W // 8])
    store = igs_model.model.diffusion_model._feature_store
    assert {k[0] for k in store} == {(0, 0), (1, 0)}, "one slot per lane"
    igs_model.model.diffusion_model.drop_feature_cache()
    assert all(torch.isfinite(v).all() for v in solo) and not torch.equal(solo[0], solo[1])
    for i in range(2):
        assert torch.equal(lanes[i], solo[i]), f"two streams: clip {i} differs from its solo cached run in {int((lanes[i] != solo[i]).sum())} elements"
        assert torch.equal(batched[i], solo[i]), f"batched: clip {i} differs from its solo cached run in {int((batched[i] != solo[i]).sum())} elements"
    monkeypatch.delenv("VCX_FEATURE_CACHE")
    from viewcrafter_amd import parallel
    from viewcrafter_amd.utils.diffusion_utils import image_guided_synthesis
    torch.manual_seed(900)
    with torch.no_grad():
        plain = image_guided_synthesis(igs_model, [""], clips[0], [1, 4, IGS_T, IGS_H // 8, IGS_W // 8], n_samples=1, ddim_steps=4, ddim_eta=1.0,
                                       unconditional_guidance_scale=7.5, cfg_img=None, fs=10, text_input=False, multiple_cond_cfg=False,
                                       timestep_spacing="uniform_trailing", guidance_rescale=0.7, condition_index=[0])
    assert not torch.equal(plain, solo[0]), "the cached run must differ from the uncached one, or this test shows nothing"


def test_two_guidance_ranks_write_the_one_process_cached_video(tmp_path):
    """`inference.py` under VCX_GUIDANCE_PARALLEL with two ranks on this box's one GPU (VCX_SHARE_GPU=1 test mode), VCX_FEATURE_CACHE=2 in
    both runs: every rank keeps the slot of its own conditioning, the video is the one-process cached video bit for bit."""
    from tests.test_guidance_parallel_gpu import _cli
    from tests.util import write_tiny_entry_files
    ypath, cpath, rpath, thw = write_tiny_entry_files(tmp_path)
    env = {"VCX_FEATURE_CACHE": "2"}
    plain = _cli(tmp_path, "plain", [rpath], ypath, cpath, thw, env_extra={"VCX_FEATURE_CACHE": "0"})[0]
    want = _cli(tmp_path, "cached", [rpath], ypath, cpath, thw, env_extra=env)[0]
    got, stdout = _cli(tmp_path, "cached_split2", [rpath], ypath, cpath, thw, ranks=2, env_extra=env)
    assert stdout.count("[guidance-parallel] 1 groups of 2: [[0, 1]], idle []") == 1, stdout[-2000:]
    assert torch.equal(got[0], want[0]), f"{int((got[0] != want[0]).sum())} elements differ"
    assert not torch.equal(want[0], plain[0]) and torch.isfinite(want[0]).all()

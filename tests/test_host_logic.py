"""CPU tests of the host-side logic: config/plugin mechanism, schedules and sampler tables against the reference's golden
vectors, state-dict contract, checkpoint loader, weight packing, and the no-fallback rule."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.tiny_config import TINY_DDCONFIG, TINY_UNET, tiny_model_params
from tests.util import golden
from viewcrafter_amd.config import Config, load_yaml
from viewcrafter_amd.utils import diffusion_utils as du

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tiny_model():
    params = Config.wrap(tiny_model_params("lvdm.modules.networks.openaimodel3d.UNetModel", "lvdm.models.autoencoder.AutoencoderKL"))
    return du.instantiate_from_config(Config(target="lvdm.models.ddpm3d.VIPLatentDiffusion", params=params)).eval()


# ------------------------------------------------------------------ config / plugin mechanism
def test_config_container_supports_both_access_styles():
    c = Config.wrap({"a": {"b": [1, {"c": 2}]}, "target": "x"})
    assert c.a.b[1].c == 2 and c["a"]["b"][0] == 1 and "target" in c and c.get("zzz") is None
    with pytest.raises(AttributeError):
        c.missing


def test_instantiate_from_config_contract():
    assert du.instantiate_from_config("__is_first_stage__") is None
    assert du.instantiate_from_config("__is_unconditional__") is None
    with pytest.raises(KeyError):
        du.instantiate_from_config({"params": {}})
    lin = du.instantiate_from_config({"target": "torch.nn.Linear", "params": {"in_features": 3, "out_features": 2}})
    assert isinstance(lin, torch.nn.Linear)
    from viewcrafter_amd.lvdm.models.autoencoder import AutoencoderKL
    assert du.get_obj_from_str("lvdm.models.autoencoder.AutoencoderKL") is AutoencoderKL      # reference path -> ours


@pytest.mark.parametrize("name,size,scale", [("inference_pvd_1024.yaml", [72, 128], 0.3), ("inference_pvd_512.yaml", [40, 64], 0.7)])
def test_shipped_yaml_graphs(name, size, scale):
    cfg = load_yaml(os.path.join(ROOT, "configs", name))
    p = cfg.model.params
    assert cfg.model.target == "lvdm.models.ddpm3d.VIPLatentDiffusion"
    assert p.image_size == size and p.base_scale == scale and p.parameterization == "v" and p.rescale_betas_zero_snr
    u = p.unet_config.params
    assert (u.in_channels, u.model_channels, u.num_head_channels, u.context_dim, u.temporal_length) == (8, 320, 64, 1024, 16)
    assert p.first_stage_config.params.ddconfig.ch_mult == [1, 2, 4, 4]


# ------------------------------------------------------------------ schedules vs the reference's golden vectors
def test_schedule_functions_match_reference():
    from viewcrafter_amd.lvdm.models import utils_diffusion as ud
    g = golden("schedules")
    betas = ud.make_beta_schedule("linear", 1000, linear_start=0.00085, linear_end=0.012)
    assert np.array_equal(betas, g["betas_linear"])
    assert np.allclose(ud.rescale_zero_terminal_snr(betas), g["betas_zero_snr"], rtol=0, atol=1e-15)
    for other in ("cosine", "sqrt_linear", "sqrt"):
        assert np.array_equal(np.asarray(ud.make_beta_schedule(other, 1000, linear_start=0.00085, linear_end=0.012), dtype=np.float64),
                              g[f"betas_{other}"]), other
    with pytest.raises(ValueError):
        ud.make_beta_schedule("nope", 1000)
    for method, n in (("uniform_trailing", 50), ("uniform_trailing", 5), ("uniform_trailing", 10), ("uniform", 50), ("quad", 20)):
        assert np.array_equal(ud.make_ddim_timesteps(method, n, 1000, verbose=False), g[f"ddim_timesteps_{method}_{n}"])
    with pytest.raises(NotImplementedError):
        ud.make_ddim_timesteps("nope", 5, 1000, verbose=False)
    acp = torch.tensor(np.cumprod(1.0 - g["betas_zero_snr"]), dtype=torch.float32)
    for eta in (0.0, 1.0):
        s, a, ap = ud.make_ddim_sampling_parameters(acp, g["ddim_timesteps_uniform_trailing_50"], eta, verbose=False)
        assert np.allclose(s, g[f"ddim_sigmas_eta{eta}"], rtol=1e-6, atol=1e-9)
        assert np.allclose(a, g[f"ddim_alphas_eta{eta}"], rtol=1e-7) and np.allclose(ap, g[f"ddim_alphas_prev_eta{eta}"], rtol=1e-7)
    from oracle.weights import synth_input
    a, b = synth_input("cfg_a", (2, 4, 3, 8, 8)), synth_input("cfg_b", (2, 4, 3, 8, 8))
    assert np.allclose(ud.rescale_noise_cfg(a, b, 0.7).numpy(), g["rescale_noise_cfg"], atol=1e-6)
    # VAE posterior (lvdm/distributions.py:24-65): sample with supplied noise, kl to N(0, 1) and to another posterior, nll
    from viewcrafter_amd.lvdm.distributions import DiagonalGaussianDistribution
    post = DiagonalGaussianDistribution(synth_input("gauss_moments", (2, 8, 4, 6), scale=3.0))
    other = DiagonalGaussianDistribution(synth_input("gauss_moments2", (2, 8, 4, 6), scale=1.5))
    x = post.sample(noise=synth_input("gauss_noise", (2, 4, 4, 6)))
    for have, key in ((x, "gauss_sample"), (post.kl(), "gauss_kl"), (post.kl(other), "gauss_kl_other"), (post.nll(x), "gauss_nll")):
        assert np.allclose(have.numpy(), g[key], rtol=1e-6, atol=1e-6), key
    det = DiagonalGaussianDistribution(synth_input("gauss_moments", (2, 8, 4, 6)), deterministic=True)
    assert torch.equal(det.sample(), det.mode()) and float(det.kl()) == 0.0 and float(det.nll(x)) == 0.0


def test_model_buffers_and_sampler_tables_match_reference(tiny_model):
    from viewcrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    g = golden("ddim_tiny")
    for k in ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "scale_arr"):
        assert np.array_equal(getattr(tiny_model, k).numpy(), g["model_" + k]), k
    assert tiny_model.num_timesteps == 1000 and tiny_model.parameterization == "v" and tiny_model.use_dynamic_rescale
    assert tiny_model.model.conditioning_key == "hybrid" and tiny_model.uncond_type == "empty_seq" and tiny_model.perframe_ae
    assert tiny_model.model.diffusion_model.out_channels == 4
    s = DDIMSampler(tiny_model)
    s.make_schedule(5, ddim_discretize="uniform_trailing", ddim_eta=0.0, verbose=False)
    assert list(s.ddim_timesteps) == list(g["ddim_timesteps"]) == [199, 399, 599, 799, 999]
    assert np.allclose(s.ddim_scale_arr.numpy(), g["ddim_scale_arr"]) and np.allclose(s.ddim_scale_arr_prev.numpy(), g["ddim_scale_arr_prev"])
    # zero terminal SNR: the first step has a_t == 0 exactly and the direction coefficient stays real
    assert float(s._host["a"][-1]) == 0.0 and float(1.0 - s._host["a_prev"][-1] - s._host["sigma"][-1] ** 2) >= 0.0


# ------------------------------------------------------------------ state-dict contract (strict checkpoint loading)
def test_state_dict_names_and_shapes_equal_the_reference(tiny_model):
    from viewcrafter_amd.lvdm.models.autoencoder import AutoencoderKL
    from viewcrafter_amd.lvdm.modules.networks.openaimodel3d import UNetModel
    for fixture, keys, shapes, module in (
            ("unet_tiny", "unet_keys", "unet_shapes", UNetModel(**TINY_UNET)),
            ("vae_tiny", "vae_keys", "vae_shapes", AutoencoderKL(ddconfig=TINY_DDCONFIG, lossconfig=None, embed_dim=4)),
            ("ddim_tiny", "model_keys", "model_shapes", tiny_model)):
        g = golden(fixture)
        ref = {str(k): eval(str(s)) for k, s in zip(g[keys], g[shapes])}
        mine = {k: tuple(v.shape) for k, v in module.state_dict().items()}
        assert mine == ref, (fixture, sorted(set(ref) ^ set(mine))[:5])
    sd = tiny_model.state_dict()
    assert sd["model.diffusion_model.init_attn.0.proj_in.weight"].dim() == 3          # Conv1d projection
    assert "model.diffusion_model.input_blocks.1.0.temopral_conv.conv2.3.weight" in sd  # (sic) + Dropout index shift


@pytest.mark.parametrize("cfg", ["inference_pvd_1024", "inference_pvd_512"])
def test_full_size_state_dict_contract(cfg):
    """At the sizes of the shipped YAMLs (1.44 B-parameter UNet: 1516 entries; VAE 248; Resampler 51) every parameter / buffer name
    and shape equals what the reference's modules register (tests/golden/state_dict_full.npz, written by the imported reference on
    the meta device): a real ViewCrafter checkpoint loads with strict=True.  Built on the meta device here too (no memory)."""
    from viewcrafter_amd.lvdm.models.autoencoder import AutoencoderKL
    from viewcrafter_amd.lvdm.modules.encoders.resampler import Resampler
    from viewcrafter_amd.lvdm.modules.networks.openaimodel3d import UNetModel
    mp = load_yaml(os.path.join(ROOT, "configs", cfg + ".yaml"))["model"]["params"]
    g = golden("state_dict_full")
    with torch.device("meta"):
        mods = {"unet": UNetModel(**dict(mp["unet_config"]["params"])),
                "vae": AutoencoderKL(**dict(mp["first_stage_config"]["params"])),
                "resampler": Resampler(**dict(mp["image_proj_stage_config"]["params"]))}
    counts = {}
    for name, m in mods.items():
        ref = {str(k): tuple(int(d) for d in str(s).split(",") if d) for k, s in zip(g[f"{cfg}__{name}__keys"], g[f"{cfg}__{name}__shapes"])}
        mine = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        assert mine == ref, (name, sorted(set(ref) ^ set(mine))[:5], [(k, ref[k], mine[k]) for k in ref if k in mine and ref[k] != mine[k]][:5])
        counts[name] = (len(mine), sum(int(np.prod(s)) if s else 1 for s in mine.values()))
    assert counts["unet"][0] == 1516 and abs(counts["unet"][1] / 1e6 - 1438.85) < 0.01
    assert counts["vae"][0] == 248 and counts["resampler"][0] == 51


def test_zero_initialised_layers_like_the_reference():
    from viewcrafter_amd.lvdm.modules.networks.openaimodel3d import UNetModel
    m = UNetModel(**TINY_UNET)
    sd = m.state_dict()
    for k in ("out.2.weight", "input_blocks.1.0.out_layers.3.weight", "input_blocks.1.0.temopral_conv.conv4.3.weight",
              "input_blocks.1.1.proj_out.weight", "input_blocks.1.2.proj_out.weight", "fps_embedding.2.weight"):
        assert float(sd[k].abs().max()) == 0.0, k


def test_load_model_checkpoint_layouts(tmp_path, tiny_model):
    from viewcrafter_amd.lvdm.models.autoencoder import AutoencoderKL
    src = AutoencoderKL(ddconfig=TINY_DDCONFIG, lossconfig=None, embed_dim=4)
    sd = {k: torch.randn_like(v) for k, v in src.state_dict().items()}
    dst = AutoencoderKL(ddconfig=TINY_DDCONFIG, lossconfig=None, embed_dim=4)
    p1 = str(tmp_path / "lightning.ckpt")
    torch.save({"state_dict": sd, "epoch": 3, "hyper": {"x": object}}, p1)
    du.load_model_checkpoint(dst, p1)
    assert all(torch.equal(dst.state_dict()[k], v) for k, v in sd.items())
    p2 = str(tmp_path / "deepspeed.ckpt")
    torch.save({"module": {"_forward_module." + k: v * 2 for k, v in sd.items()}}, p2)
    du.load_model_checkpoint(dst, p2)
    assert all(torch.equal(dst.state_dict()[k], 2 * v) for k, v in sd.items())
    bad = dict(sd)
    bad.pop(next(iter(bad)))
    p3 = str(tmp_path / "bad.ckpt")
    torch.save({"state_dict": bad}, p3)
    with pytest.raises(RuntimeError):
        du.load_model_checkpoint(dst, p3)            # strict: a missing key is an error, as in the reference
    # 256-model rename retry: framestride_embed -> fps_embedding
    full = {k.replace("fps_embedding", "framestride_embed"): v for k, v in tiny_model.state_dict().items()}
    p4 = str(tmp_path / "renamed.ckpt")
    torch.save({"state_dict": full}, p4)
    du.load_model_checkpoint(tiny_model, p4)


# ------------------------------------------------------------------ weight packing
def test_pack_conv_is_the_im2col_order_of_the_channels_last_gather():
    from viewcrafter_amd.packing import pack_conv, pad_cin
    x = torch.randn(2, 5, 6, 8)                                           # n h w c
    w = torch.randn(4, 8, 3, 3)
    ref = F.conv2d(x.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    cols = torch.stack([xp[:, ky:ky + 5, kx:kx + 6, :] for ky in range(3) for kx in range(3)], dim=3)   # n h w tap c
    out = cols.reshape(2, 5, 6, 72) @ pack_conv(w).t()
    assert torch.allclose(out, ref, atol=1e-4)
    w3 = torch.randn(4, 8, 3, 1, 1)
    assert torch.equal(pack_conv(w3), w3[:, :, :, 0, 0].permute(0, 2, 1).reshape(4, 24))
    assert pad_cin(torch.ones(2, 4, 3, 3), 8)[:, 4:].abs().sum() == 0 and pad_cin(w, 8) is w


def test_pack_geglu_pairs_x_and_gate_in_blocks_of_32():
    from viewcrafter_amd.packing import pack_geglu
    d = 64
    w = torch.arange(2 * d, dtype=torch.float32)[:, None].repeat(1, 4)
    b = torch.arange(2 * d, dtype=torch.float32)
    wp, bp = pack_geglu(w, b)
    for blk in range(d // 32):
        assert torch.equal(bp[64 * blk:64 * blk + 32], b[32 * blk:32 * blk + 32])                 # x rows
        assert torch.equal(bp[64 * blk + 32:64 * blk + 64], b[d + 32 * blk:d + 32 * blk + 32])     # their gates
    assert torch.equal(wp[:, 0], bp)


# ------------------------------------------------------------------ sampler host logic
def test_cfg_batching_rules():
    from viewcrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    c = {"c_crossattn": [torch.zeros(1, 5, 4)], "c_concat": [torch.zeros(1, 4, 2, 2, 2)]}
    uc = {"c_crossattn": [torch.ones(1, 5, 4)], "c_concat": [torch.zeros(1, 4, 2, 2, 2)]}
    assert DDIMSampler._batchable(c, uc)
    assert not DDIMSampler._batchable(c, {"c_crossattn": [torch.ones(1, 6, 4)], "c_concat": c["c_concat"]})
    assert not DDIMSampler._batchable(c, torch.zeros(1))
    s = DDIMSampler.__new__(DDIMSampler)
    s._cfg_cache = None
    both = s._cfg_cond(c, uc)
    assert both["c_crossattn"][0].shape == (2, 5, 4) and float(both["c_crossattn"][0][1].min()) == 1.0
    assert s._cfg_cond(c, uc) is both                                   # built once per sample() call
    assert DDIMSampler._batchable(c, uc, uc) and s._cfg_cond(c, uc, uc)["c_crossattn"][0].shape == (3, 5, 4)


def test_shared_cfg_prefix_routing(tiny_model):
    """The sampler asks the UNet for the shared prefix (cfg_repeat) exactly when the conditionings differ only in c_crossattn
    (every other entry the same tensor object, as image_guided_synthesis builds them, diffusion_utils.py:132,151-153), and then
    passes x / t / fs / c_concat ONCE with the contexts stacked."""
    from viewcrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    s = DDIMSampler(tiny_model)
    cat = torch.zeros(1, 4, 2, 8, 8)
    c = {"c_crossattn": [torch.zeros(1, 77, 128)], "c_concat": [cat]}
    uc = {"c_crossattn": [torch.ones(1, 77, 128)], "c_concat": [cat]}
    uc_copy = {"c_crossattn": [torch.ones(1, 77, 128)], "c_concat": [cat.clone()]}
    assert s._shares_prefix((c, uc)) and s._shares_prefix((c, uc, uc)) and not s._shares_prefix((c, uc_copy))
    calls = []

    def spy(x, t, cond, **kw):
        calls.append((tuple(x.shape), tuple(t.shape), tuple(cond["c_crossattn"][0].shape), tuple(cond["c_concat"][0].shape),
                      kw.get("cfg_repeat"), None if kw.get("fs") is None else tuple(kw["fs"].shape)))
        return torch.zeros(cond["c_crossattn"][0].shape[0], *x.shape[1:])
    s.model = type("M", (), {"apply_model": staticmethod(spy), "model": tiny_model.model})()
    x, t, fs = torch.zeros(1, 4, 2, 8, 8), torch.tensor([5]), torch.tensor([10])
    out = s._apply_batched(x, t, (c, uc), {"fs": fs})
    assert calls[-1] == ((1, 4, 2, 8, 8), (1,), (2, 77, 128), (1, 4, 2, 8, 8), 2, (1,)) and len(out) == 2
    s._cfg_cache = None
    s._apply_batched(x, t, (c, uc_copy), {"fs": fs})                      # not shareable: plain B = 2 batch
    assert calls[-1] == ((2, 4, 2, 8, 8), (2,), (2, 77, 128), (2, 4, 2, 8, 8), None, (2,))
    s.share_cfg_prefix, s._cfg_cache = False, None
    s._apply_batched(x, t, (c, uc), {"fs": fs})
    assert calls[-1][4] is None and calls[-1][0] == (2, 4, 2, 8, 8)


# ------------------------------------------------------------------ the product has no CPU / oracle fallback
def test_forward_fails_loudly_without_gpu(tiny_model):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from viewcrafter_amd._lib import VcxError
    x = torch.zeros(1, 4, 2, 8, 8)
    cond = {"c_crossattn": [torch.zeros(1, 77, TINY_UNET["context_dim"])], "c_concat": [torch.zeros(1, 4, 2, 8, 8)]}
    with pytest.raises(VcxError):
        tiny_model.apply_model(x, torch.tensor([10]), cond)
    with pytest.raises(VcxError):
        tiny_model.decode_first_stage(torch.zeros(1, 4, 2, 8, 8))


def test_product_never_imports_the_oracle():
    offenders = []
    for base in ("viewcrafter_amd", "configs"):
        for dp, _, files in os.walk(os.path.join(ROOT, base)):
            for f in files:
                if f.endswith((".py", ".hip", ".h")):
                    src = open(os.path.join(dp, f)).read()
                    if re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M):
                        offenders.append(os.path.join(dp, f))
    for f in ("viewcrafter.py", "inference.py"):
        if re.search(r"^\s*(from|import)\s+oracle\b", open(os.path.join(ROOT, f)).read(), flags=re.M):
            offenders.append(f)
    assert not offenders, offenders


def test_multicond_sampler_schedule_uses_the_unfixed_scale_arr_prev(tiny_model):
    from viewcrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    from viewcrafter_amd.lvdm.models.samplers.ddim_multiplecond import DDIMSampler as Multi
    g = golden("ddim_tiny")
    a, m = DDIMSampler(tiny_model), Multi(tiny_model)
    a.make_schedule(5, ddim_discretize="uniform_trailing", ddim_eta=0.0, verbose=False)
    m.make_schedule(5, ddim_discretize="uniform_trailing", ddim_eta=0.0, verbose=False)
    assert np.allclose(m.ddim_scale_arr_prev.numpy(), g["multicond_scale_arr_prev"])
    assert float(a.ddim_scale_arr_prev[0]) == 1.0 and float(m.ddim_scale_arr_prev[0]) == float(m.ddim_scale_arr[0])
    assert np.allclose(m._host["ratio"], (m.ddim_scale_arr_prev / m.ddim_scale_arr).numpy())


def test_image_proj_model_resolves_natively_with_reference_state_dict_names():
    """TARGET_ALIASES maps the YAML's Resampler target onto the libvcx implementation; its parameter names / shapes are
    the reference's (pinned by the fixture written from the imported reference module)."""
    import numpy as np
    import os
    from viewcrafter_amd.config import Config
    from viewcrafter_amd.utils.diffusion_utils import instantiate_from_config
    from tests.tiny_config import TINY_RESAMPLER
    m = instantiate_from_config(Config(target="lvdm.modules.encoders.resampler.Resampler", params=Config.wrap(dict(TINY_RESAMPLER))))
    assert type(m).__module__ == "viewcrafter_amd.lvdm.modules.encoders.resampler"
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "resampler_tiny.npz"))
    want = {str(k): eval(str(s)) for k, s in zip(g["resampler_keys"], g["resampler_shapes"])}
    have = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert have == want


def test_clip_encoders_resolve_natively_with_reference_state_dict_names():
    """The YAML targets of the two OpenCLIP encoders resolve to the libvcx implementation; parameter names / shapes equal
    those of the reference modules (fixture written by the reference's condition.py on the open_clip stand-in)."""
    import numpy as np
    import os
    from viewcrafter_amd.config import Config
    from viewcrafter_amd.utils.diffusion_utils import instantiate_from_config
    from viewcrafter_amd.lvdm.modules.encoders import condition as cond
    from tests.tiny_config import CLIP_TINY, CLIP_TINY_CFG
    cond.CLIP_CONFIGS[CLIP_TINY] = CLIP_TINY_CFG
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "clip_tiny.npz"))
    for target, params, key in (("FrozenOpenCLIPEmbedder", dict(arch=CLIP_TINY, freeze=True, layer="penultimate"), "clip_text"),
                                ("FrozenOpenCLIPImageEmbedderV2", dict(arch=CLIP_TINY, freeze=True), "clip_image")):
        m = instantiate_from_config(Config(target="lvdm.modules.encoders.condition." + target, params=Config.wrap(params)))
        assert type(m).__module__ == "viewcrafter_amd.lvdm.modules.encoders.condition"
        want = {str(k): eval(str(s)) for k, s in zip(g[key + "_keys"], g[key + "_shapes"])}
        have = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        assert have == want, (sorted(set(have) ^ set(want)))
        assert not any(p.requires_grad for p in m.parameters())


def test_clip_tokenizer_contract(tmp_path, monkeypatch):
    """Empty prompt -> <start_of_text><end_of_text>; a non-empty prompt without a vocabulary fails loudly; with a (toy)
    vocabulary file the byte-pair merges are applied in rank order and long prompts are truncated with the end token kept."""
    import gzip
    import pytest
    from viewcrafter_amd.lvdm.modules.encoders import condition as cond
    monkeypatch.delenv("VCX_CLIP_BPE", raising=False)
    cond._bpe_from_env.cache_clear()
    t = cond.tokenize(["", ""])
    assert t.shape == (2, 77) and t[0, :3].tolist() == [49406, 49407, 0] and int(t.sum()) == 2 * (49406 + 49407)
    try:
        import open_clip  # noqa: F401
        return
    except ImportError:
        pass
    with pytest.raises(RuntimeError, match="VCX_CLIP_BPE"):
        cond.tokenize(["a view"])
    merges = ["#version: toy", "v i", "vi e", "vie w</w>", "a b"] + [f"x{i} y{i}" for i in range(49152 - 256 - 2 - 4)]
    path = tmp_path / "bpe.txt.gz"
    with gzip.open(path, "wb") as f:
        f.write("\n".join(merges).encode())
    monkeypatch.setenv("VCX_CLIP_BPE", str(path))
    cond._bpe_from_env.cache_clear()
    bpe = cond._bpe_from_env()
    byte = cond._bytes_to_unicode()
    ids = cond.tokenize(["A  View"])[0].tolist()
    assert ids[0] == 49406 and ids[3] == 49407 and ids[4] == 0
    assert ids[1] == bpe.encoder[byte[ord("a")] + "</w>"]                 # single letter word: its </w> symbol
    assert ids[2] == bpe.encoder["view</w>"] == 512 + 2                     # merged by the three toy merges
    long = cond.tokenize(["a " * 200])[0]
    assert long[-1] == 49407 and long[0] == 49406 and (long[1:-1] == ids[1]).all()
    cond._bpe_from_env.cache_clear()


def test_bpe_tokenizer_matches_transformers_clip_tokenizer(tmp_path, monkeypatch):
    """Non-empty prompts with $VCX_CLIP_BPE (reference condition.py:209-214 -> open_clip.tokenize): the byte-pair tokenizer against
    an independent third-party implementation of CLIP's tokenisation that IS in the image - transformers' CLIPTokenizer (Rust
    `tokenizers` backend) - given the same vocabulary and merges (learned from a small corpus, tests/util.py::write_synthetic_bpe;
    the real vocabulary file is data that is not available offline).  Lower-casing, whitespace collapsing, apostrophe / digit /
    punctuation splitting, rank-ordered merges, </w> word ends, <start_of_text> / <end_of_text> ids, truncation at 77."""
    import pytest
    pytest.importorskip("transformers")
    try:
        import open_clip  # noqa: F401
        pytest.skip("open_clip is installed: tokenize() delegates to it")
    except ImportError:
        pass
    from transformers import CLIPTokenizer
    from tests.util import write_synthetic_bpe
    from viewcrafter_amd.lvdm.modules.encoders import condition as cond
    path = str(tmp_path / "bpe_syn.txt.gz")
    merges = write_synthetic_bpe(path)
    monkeypatch.setenv("VCX_CLIP_BPE", path)
    cond._bpe_from_env.cache_clear()
    try:
        bpe = cond._bpe_from_env()
        vocab = dict(bpe.encoder)
        vocab["<|startoftext|>"], vocab["<|endoftext|>"] = vocab.pop("<start_of_text>"), vocab.pop("<end_of_text>")
        assert vocab["<|startoftext|>"] == 49406 and vocab["<|endoftext|>"] == 49407 and len(vocab) == 49408
        hf = CLIPTokenizer(vocab=vocab, merges=[tuple(m) for m in merges])
        prompts = ["A photo of a large room", "the artist's view , camera moving forward .", "naive cafe 22 chairs !!", "  wooden   Furniture ",
                   "a sweeping view of the old town at night, 4k, highly detailed", "it's", "a " * 100, "view" * 40]
        merged_tokens = 0
        for p in prompts:
            ours = cond.tokenize([p])[0].tolist()
            theirs = hf(p, padding="max_length", max_length=77, truncation=True)["input_ids"]
            end = theirs.index(49407)
            theirs = [t if i <= end else 0 for i, t in enumerate(theirs)]          # HF pads with <end_of_text>, open_clip with 0
            assert ours == theirs, (p, ours[:16], theirs[:16])
            merged_tokens += sum(1 for t in ours if 512 <= t < 49406)
        assert merged_tokens > 20                                                   # the merges were exercised, not only single bytes
    finally:
        cond._bpe_from_env.cache_clear()


def test_fold_layernorm_is_the_exact_algebra_of_layernorm_then_linear():
    """packing.fold_layernorm (VCX_GEMM_LNFOLD, include/vcx.h): with the ROUNDED fp16 weights w', colsum = their fp32 row sums and
    bias' = bias + w beta,  rstd (x w'^T - mean colsum) + bias'  IS  LayerNorm(x) w^T + bias  up to the fp16 rounding of gamma o w -
    for rows with any common offset, because x w'^T - mean colsum = sum_k (x_k - mean) w'_k term by term.  fp64 on the host."""
    from viewcrafter_amd.packing import fold_layernorm, pack_geglu
    g = torch.Generator().manual_seed(5)
    K, N = 128, 96
    w, bias = torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g) * 0.1
    gamma, beta = 1 + 0.3 * torch.randn(K, generator=g), 0.2 * torch.randn(K, generator=g)
    wf, colsum, bias_f = fold_layernorm(w, gamma, beta, bias)
    assert wf.dtype == torch.float16 and colsum.dtype == bias_f.dtype == torch.float32
    assert torch.equal(colsum, wf.double().sum(1).float())              # of the rounded weights, not of gamma o w
    for offset in (0.0, 900.0):
        x = (torch.randn(50, K, generator=g) * 8 + offset).half().double()
        mean, var = x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
        rstd = 1.0 / torch.sqrt(var + 1e-5)
        folded = rstd * (x @ wf.double().t() - mean * colsum.double()) + bias_f.double()
        exact_for_wf = ((x - mean) * rstd) @ wf.double().t() + bias_f.double()            # same weights: identical up to fp64 rounding
        # colsum is held in fp32: the residue is |mean| rstd ulp32(colsum) / 2 ~ 900 / 8 x 6e-8 at offset 900 (fp16 output ulp: 5e-4)
        assert float((folded - exact_for_wf).abs().max()) <= (2e-5 if offset else 1e-7)
        ref = ((x - mean) * rstd * gamma.double() + beta.double()) @ w.double().t() + bias.double()
        assert float((folded - ref).norm() / ref.norm()) <= 5e-4                          # fp16 rounding of gamma o w only
    # GEGLU: colsum travels through pack_geglu like the bias
    w8, b8 = torch.randn(128, K, generator=g), torch.randn(128, generator=g)
    wf, colsum, bias_f = fold_layernorm(w8, gamma, beta, b8)
    wp, bp = pack_geglu(wf, bias_f)
    _, cp = pack_geglu(wf, colsum)
    assert torch.equal(cp, wp.double().sum(1).float())


def test_colstats_eligibility_mirrors_the_kernels_conditions():
    """ops.colstats_ok: GroupNorm statistics come from the producing convolution's epilogue only where the DMA conv kernel runs
    (cin % 64 == 0, cout % 8 == 0, 32-bit byte offsets) and every statistics unit is whole 64-row strips - all levels of 576x1024 and
    320x512 but the deepest (9x16 / 5x8 pixels per frame), per frame and per video; elsewhere the statistics pass stays."""
    from viewcrafter_amd import ops
    for h, w, ok in ((72, 128, True), (36, 64, True), (18, 32, True), (9, 16, False), (40, 64, True), (20, 32, True), (10, 16, False), (5, 8, False)):
        n = 50
        assert ops.colstats_ok(n * h * w, h * w, 320, 320) is ok, (h, w)                       # per frame
        assert ops.colstats_ok(n * h * w, 25 * h * w, 640, 640) is (25 * h * w % 64 == 0), (h, w)   # per video
    assert not ops.colstats_ok(50 * 72 * 128, 72 * 128, 8, 320)            # conv_in: 8 input channels -> register-staged kernel
    assert not ops.colstats_ok(50 * 72 * 128, 72 * 128, 320, 4)            # the 4-channel output convolution
    assert not ops.colstats_ok(8 * 1024 * 1024, 1024 * 1024, 320, 320)     # output beyond 32-bit byte offsets
    assert ops.colstats_ok(460800, 9216, 960, 320, in_rows=460800) and not ops.colstats_ok(460800, 9216, 960, 320, in_rows=3_000_000)


def test_pack_conv_slab_major_order_for_64_channel_multiples():
    """cin % 64 == 0 and more than one tap: K is ordered (c / 64, tap, c % 64) - VCX_GEMM_CONV_SLABK, the order both GEMM
    kernels walk when ops.conv2d / temporal_conv3 set the flag from the same predicate."""
    from oracle.weights import synth_input
    from viewcrafter_amd.packing import conv_slab_major, pack_conv
    assert conv_slab_major(320, 9) and conv_slab_major(128, 3) and not conv_slab_major(320, 1) and not conv_slab_major(8, 9)
    w = synth_input("w_slab", (5, 128, 3, 3))
    x = synth_input("x_slab", (2, 4, 6, 128))
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    cols = torch.stack([xp[:, ky:ky + 4, kx:kx + 6, :] for ky in range(3) for kx in range(3)], dim=3)     # n h w tap c
    cols = cols.view(2, 4, 6, 9, 2, 64).permute(0, 1, 2, 4, 3, 5).reshape(2, 4, 6, 9 * 128)               # n h w (slab tap c64)
    out = cols @ pack_conv(w).t()
    ref = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1)
    assert torch.allclose(out, ref, atol=1e-4)
    w1 = synth_input("w_1x1", (5, 128, 1, 1))
    assert torch.equal(pack_conv(w1), w1[:, :, 0, 0])


def test_cli_surface_equals_the_reference_parser():
    """Every `python inference.py` option of the reference (configs/infer_config.py:7-59, read from its own argparse parser into
    tests/golden/cli_flags.npz) exists here with the same type, default, nargs and action; this repo only adds options."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("vcx_infer_config", os.path.join(ROOT, "configs", "infer_config.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mine = {}
    for a in mod.get_parser()._actions:
        for opt in a.option_strings:
            if opt.startswith("--") and opt != "--help":
                mine[opt] = (getattr(a.type, "__name__", str(a.type)), repr(a.default), repr(a.nargs), type(a).__name__)
    g = golden("cli_flags")
    ref = {str(f): (str(t), str(d), str(n), str(ac)) for f, t, d, n, ac in zip(g["flag"], g["type"], g["default"], g["nargs"], g["action"])}
    assert len(ref) == 44
    assert not [f for f in ref if f not in mine], [f for f in ref if f not in mine]
    assert not {f: (ref[f], mine[f]) for f in ref if ref[f] != mine[f]}, {f: (ref[f], mine[f]) for f in ref if ref[f] != mine[f]}
    assert sorted(set(mine) - set(ref)) == ["--reference_root", "--renderings"]


def test_call_signatures_on_the_boundary_equal_the_reference():
    """65 functions / methods of the drop-in boundary: every parameter the reference declares (read from its
    source with `ast` into tests/golden/api_signatures.npz) exists here, in the same position and with the same default, and a
    reference **kwargs stays a **kwargs; this repo only ever appends parameters.  Inherited methods count (the multi-condition
    sampler subclasses DDIMSampler here)."""
    import ast
    import importlib
    import inspect
    import json
    table = json.loads(str(golden("api_signatures")["json"]))
    where = {"viewcrafter.py": "viewcrafter", "utils/diffusion_utils.py": "viewcrafter_amd.utils.diffusion_utils",
             "utils/pvd_utils.py": "viewcrafter_amd.utils.pvd_utils"}
    # defaults that are deliberately more permissive here (a required argument of the reference has a default)
    relaxed = {("lvdm/models/autoencoder.py", "AutoencoderKL.__init__"): {"lossconfig", "embed_dim"}}
    problems, checked = [], 0
    for rel, funcs in table.items():
        mod = importlib.import_module(where.get(rel, "viewcrafter_amd." + rel[:-3].replace("/", ".")))
        for qual, ref in funcs.items():
            obj = mod
            try:
                for part in qual.split("."):
                    obj = getattr(obj, part)
            except AttributeError:
                problems.append(f"{rel}:{qual} missing")
                continue
            sig = inspect.signature(obj)
            mine = list(sig.parameters.values())
            names = [p.name for p in mine]
            for pos, (name, dflt) in enumerate(ref["args"]):
                if name not in names:
                    problems.append(f"{rel}:{qual} lacks parameter {name}")
                    continue
                p = mine[names.index(name)]
                if names.index(name) != pos:
                    problems.append(f"{rel}:{qual} parameter {name} at position {names.index(name)} (reference {pos})")
                if dflt is None:
                    if p.default is not inspect.Parameter.empty and name not in relaxed.get((rel, qual), ()):
                        problems.append(f"{rel}:{qual} {name} is required in the reference")
                    continue
                if p.default is inspect.Parameter.empty:
                    problems.append(f"{rel}:{qual} {name} has no default (reference {dflt})")
                    continue
                try:
                    want = ast.literal_eval(dflt)
                except Exception:
                    continue                     # a non-literal default expression: presence and position are what is checked
                have = p.default
                same = (list(have) == list(want)) if isinstance(want, (list, tuple)) and isinstance(have, (list, tuple)) else (have == want and type(have) is type(want))
                if not same:
                    problems.append(f"{rel}:{qual} {name} default {have!r} (reference {want!r})")
            if ref["kwarg"] and not any(p.kind is inspect.Parameter.VAR_KEYWORD for p in mine):
                problems.append(f"{rel}:{qual} has no **kwargs")
            if ref["vararg"] and not any(p.kind is inspect.Parameter.VAR_POSITIONAL for p in mine):
                problems.append(f"{rel}:{qual} has no *args")
            checked += 1
    assert not problems, "\n".join(problems)
    assert checked == 65


def test_batched_posterior_noise_is_the_per_frame_stream():
    """The reference encodes the condition video frame by frame (perframe_ae) and each frame's posterior draws its own CPU noise
    (ddpm3d.py:630-637, distributions.py:35-40); here frames are encoded in one batch and the noise is ONE torch.randn over all
    frames.  torch's CPU normal fill works in blocks of 16, so the two consume the generator identically whenever a frame's latent
    has a multiple of 16 elements (4 * h * w with h * w % 4 == 0: every supported size) - a seeded run sees the reference's noise."""
    from viewcrafter_amd.lvdm.distributions import DiagonalGaussianDistribution
    for h, w in ((72, 128), (40, 64), (9, 16), (6, 10)):
        moments = torch.zeros(3, 8, h, w)
        torch.manual_seed(123)
        batched = DiagonalGaussianDistribution(moments).sample()
        torch.manual_seed(123)
        per_frame = torch.cat([DiagonalGaussianDistribution(moments[i:i + 1]).sample() for i in range(3)])
        assert torch.equal(batched, per_frame), (h, w)


def test_committed_bench_line_keeps_the_contract():
    """The newest committed bench line (profiles/r0N*_bench.json, written by `python bench.py` on an MI355X) has every field of the
    bench contract with consistent values: value = n_gpus * steps / elapsed, roofline.frac = achieved / peak, inputs HBM-resident
    synthetic data, a bounded CPU sample."""
    import glob
    import json
    paths = sorted(p for p in glob.glob(os.path.join(ROOT, "profiles", "r0[0-9]*_bench.json")) if "ViewCrafter" not in os.path.basename(p))
    assert paths
    d = json.loads(open(paths[-1]).read().strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["unit"] == "DDIM steps/s" and d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["dtype"] == "f16" and "synthetic" in d["data"] and "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - d["n_gpus"] * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    r = d["roofline"]
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and r["peak"] == 2500.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["traffic"] is None or r["traffic"] > 0
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0 and c["unit"] == d["unit"] and c["sample"]
    assert 3.0 < d["value"] < 8.0           # 576x1024x25 on one MI355X: the measured range of this code base
    assert c["kind"] == "reference" and c["vae_decode_s_per_frame"] > 0      # round 3: the reference's own code, with a VAE leg


def test_readme_and_design_quote_the_drivers_bench_record():
    """The headline in README.md / DESIGN.md is the DRIVER's measurement, not the builder's best box: both name a BENCH_rNN.json
    and quote its value and ms_per_step to the printed precision."""
    import json
    import re
    for doc in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        m = re.search(r"(BENCH_r\d+\.json)`?\)?[:,]?\s*\**([0-9.]+) DDIM steps/s(?: =|,) ([0-9.]+) ms/step", text)
        assert m, f"{doc}: no 'BENCH_rNN.json ... X DDIM steps/s ... Y ms/step' line"
        rec = json.load(open(os.path.join(ROOT, m.group(1))))["parsed"]
        assert abs(rec["value"] - float(m.group(2))) < 0.006, (doc, m.group(0), rec["value"])
        assert abs(rec["ms_per_step"] - float(m.group(3))) < 0.06, (doc, m.group(0), rec["ms_per_step"])


@pytest.mark.parametrize("name", ["inference_pvd_1024", "inference_pvd_512"])
def test_reference_yaml_selects_this_implementation(name):
    """The reference's own YAML (parsed into tests/golden/reference_yaml.npz by the generator) differs from configs/<name>.yaml
    only in training-only keys, and - unchanged, with its `lvdm.*` target strings - instantiates THIS implementation through
    instantiate_from_config: UNet, VAE, Resampler and both OpenCLIP encoders, built here on the meta device."""
    import json
    ref = json.loads(str(golden("reference_yaml")[name]))
    mine = load_yaml(os.path.join(ROOT, "configs", name + ".yaml"))
    mine = json.loads(json.dumps(mine.to_dict() if hasattr(mine, "to_dict") else mine, default=lambda o: dict(o)))
    diffs = []

    def walk(x, y, path):
        if isinstance(x, dict) and isinstance(y, dict):
            for k in sorted(set(x) | set(y)):
                if k not in x or k not in y:
                    diffs.append(path + "/" + k)
                else:
                    walk(x[k], y[k], path + "/" + k)
        elif x != y:
            diffs.append(path)
    walk(ref, mine, "")
    allowed = {"/model/base_learning_rate", "/model/pretrained_checkpoint", "/model/scale_lr", "/model/params/loop_video"}
    assert set(diffs) <= allowed, sorted(set(diffs) - allowed)
    mp = Config.wrap(ref["model"])
    assert mp["target"] == "lvdm.models.ddpm3d.VIPLatentDiffusion"
    with torch.device("meta"):
        model = du.instantiate_from_config(mp)
    assert type(model).__module__.startswith("viewcrafter_amd.")
    for sub in (model.model.diffusion_model, model.first_stage_model, model.image_proj_model, model.cond_stage_model, model.embedder):
        assert type(sub).__module__.startswith("viewcrafter_amd."), type(sub)
    assert model.model.conditioning_key == "hybrid" and model.parameterization == "v" and model.use_dynamic_rescale
    assert sum(p.numel() for p in model.model.diffusion_model.parameters()) == 1438854980        # SURVEY: 1438.85 M
    assert sum(p.numel() for p in model.parameters()) == 2609129005


def test_folded_packs_follow_the_parent_blocks_layernorm_and_lnfold_ok_mirrors_the_kernel(monkeypatch):
    """the packed projection weights of CrossAttention embed the LayerNorm of the OWNING BasicTransformerBlock; changing
    that norm by any route (`.data` assignment, in-place edit, norm.load_state_dict) must rebuild them - they used to be dropped only
    through the block's own _apply / load_state_dict hooks.  And ops.lnfold_ok says where the folded kernel applies, so that a shape
    outside it takes LayerNorm + the plain projection instead of VCX_EINVAL from every transformer block."""
    from viewcrafter_amd import ops
    from viewcrafter_amd.lvdm.modules import attention as A
    torch.manual_seed(0)
    blk = A.BasicTransformerBlock(128, 2, 64, context_dim=None)
    blk.set_kind("temporal")
    with torch.no_grad():
        blk.norm1.weight.copy_(1 + 0.1 * torch.randn(128))
    first = blk.attn1.packed()
    assert first["qkv"]["colsum"] is not None and blk.attn1.packed() is first            # folded, and cached
    w0 = first["qkv"]["w"].clone()
    with torch.no_grad():
        blk.norm1.weight.mul_(2.0)                                                        # in place: version counter moves
    second = blk.attn1.packed()
    assert second is not first and torch.allclose(second["qkv"]["w"].float(), 2 * w0.float(), rtol=2e-3, atol=1e-4)
    blk.norm1.weight.data = torch.ones(128)                                               # storage swapped under the parameter
    third = blk.attn1.packed()
    assert third is not second and not torch.equal(third["qkv"]["w"], second["qkv"]["w"])
    blk.norm1.load_state_dict({"weight": torch.full((128,), 0.5), "bias": torch.zeros(128)})
    assert blk.attn1.packed() is not third
    # the un-folded form of a folded pack, built on demand, is the plain fp16 weight
    plain_w, plain_b = A._plain_of(blk.attn1.packed()["qkv"])
    assert plain_b is None and torch.equal(plain_w, torch.cat([blk.attn1.to_q.weight, blk.attn1.to_k.weight, blk.attn1.to_v.weight]).detach().half())
    # lnfold_ok: mirrors dma_ok of csrc/gemm.hip (knob, K % 64, GEMM N % 8, 32-bit extents incl. 256 rows past the end)
    assert ops.tune_get("GEMM_DMA") == 1
    assert ops.lnfold_ok(460800, 960, 320) and ops.lnfold_ok(460800, 320, 320, transposed=True)
    assert not ops.lnfold_ok(460800, 960, 72)                       # K % 64
    assert not ops.lnfold_ok(1001, 320, 320, transposed=True)       # GEMM N = tokens % 8
    assert not ops.lnfold_ok(3_500_000, 960, 640)                   # 4.5 GB of token rows: beyond 32-bit byte offsets
    assert not ops.lnfold_ok(1_200_000, 2560, 320)                  # output rows x ldc beyond 4 GiB
    ops.tune_set("GEMM_DMA", 0)
    try:
        assert not ops.lnfold_ok(460800, 960, 320)                  # knob GEMM_DMA = 0: register-staged kernel, no folded epilogue
    finally:
        ops.tune_set("GEMM_DMA", 1)


# ------------------------------------------------------------------ batch invariance of the host's route decisions (full width, no GPU)
class _RouteRecorder:
    """Shape-only stand-ins for the ops launchers that record, per launch, what selects a kernel route: the entry point, rows per unit,
    which by-products (row statistics, column moments, folded LayerNorm statistics, K tail) are asked for.  Activations live on the
    meta device, so the full-width blocks of the 1.44 B model run in milliseconds without allocating a byte."""

    def __init__(self):
        self.log = []

    def install(self, monkeypatch):
        from viewcrafter_amd import _lib, ops
        meta = torch.device("meta")
        rec = self.log.append

        def gemm(a, w, *, M, N, K, out=None, geglu=False, out_f32=False, conv=None, ln_stats=None, colstats=None, rowstats=None, tail=None,
                 residual=None, rowadd=None, bias_m=False, **kw):
            rec(("gemm", "conv" if conv else "linear", M if bias_m else N, K, geglu, ln_stats is not None, colstats is not None, rowstats is not None,
                 len(tail or ()), residual is not None, rowadd is not None))      # (N of the transposed V^T projection counts tokens)
            n_out = N // 2 if geglu else N
            return out if out is not None else torch.empty((M, n_out), dtype=torch.float32 if out_f32 else torch.float16, device=meta)

        def gemm_units(a, wn, bn, *, unit_rows, out=None, rowstats=None, rowstats_eps=1e-5):
            rec(("gemm_units", unit_rows, rowstats is not None))
            return out if out is not None else torch.empty((a.shape[0], wn.shape[1]), dtype=torch.float16, device=meta)

        def gn_stats(x, groups=32):
            rec(("group_norm_stats", x.shape[1]))
            return torch.empty((x.shape[0], groups, 2), device=meta)

        def gn_from_cs(cs, n_outer, pixels, C, groups=32):
            rec(("group_norm_stats_from_colstats", pixels, C))
            return torch.empty((n_outer, groups, 2), device=meta)

        def gn_fold(w32, bias, gamma, beta, stats, eps, groups=32):
            rec(("group_norm_fold_linear",))
            n, (N, C) = stats.shape[0], w32.shape
            return torch.empty((n, N, C), dtype=torch.float16, device=meta), torch.empty((n, N), device=meta)

        def group_norm(x, gamma, beta, eps, silu, groups=32, out=None, stats=None, x2=None):
            rec(("group_norm", x.shape[1], stats is not None, x2 is not None))
            C = x.shape[2] + (0 if x2 is None else x2.shape[2])
            return out if out is not None else torch.empty((x.shape[0], x.shape[1], C), dtype=torch.float16, device=meta)

        def row_stats(x, eps=1e-5):
            rec(("row_stats",))
            return torch.empty((x.shape[0], 2), device=meta)

        def layer_norm(x, gamma, beta, eps=1e-5):
            rec(("layer_norm",))
            return torch.empty_like(x)

        def attention(name):
            def run(*a, **kw):
                rec((name, kw.get("nq"), kw.get("T"), kw.get("P")))
                return a[3] if name == "flash_attn" else (a[5] if name == "flash_attn_dual" else a[1])
            return run
        table = dict(require_gpu=lambda: None, gemm=gemm, gemm_units=gemm_units, group_norm_stats=gn_stats, group_norm_stats_from_colstats=gn_from_cs,
                     group_norm_fold_linear=gn_fold, group_norm=group_norm, row_stats=row_stats, layer_norm=layer_norm,
                     flash_attn=attention("flash_attn"), flash_attn_dual=attention("flash_attn_dual"), temporal_attn=attention("temporal_attn"),
                     copy2d=lambda *a, **k: None, tune_get=lambda name: _lib.TUNE[name][1])
        for name, fn in table.items():
            monkeypatch.setattr(ops, name, fn)


def _meta_unet(yaml_name):
    from viewcrafter_amd.lvdm.modules.networks.openaimodel3d import UNetModel
    params = dict(load_yaml(os.path.join(ROOT, "configs", yaml_name))["model"]["params"]["unet_config"]["params"])
    params["use_checkpoint"] = False
    with torch.device("meta"):
        return UNetModel(**params).eval()


_UNETS = {}


def _block_routes(monkeypatch, yaml_name, level, B, T, h, w, r=1):
    """The launches of input block 1 (level 0, C = 320) or 4 (level 1, C = 640) - ResBlock, SpatialTransformer (shared CFG prefix when
    r > 1), TemporalTransformer - for B videos of T x h x w latents (level 1: h / 2 x w / 2)."""
    from viewcrafter_amd.lvdm.modules.attention import SpatialTransformer
    if yaml_name not in _UNETS:
        _UNETS[yaml_name] = _meta_unet(yaml_name)
    unet = _UNETS[yaml_name]
    blk = unet.input_blocks[1 if level == 0 else 4]
    rb, st, tt = list(blk)
    rec = _RouteRecorder()
    rec.install(monkeypatch)
    meta = torch.device("meta")
    hh, ww = (h, w) if level == 0 else (h // 2, w // 2)
    x = torch.empty((B * T, hh, ww, rb.channels), dtype=torch.float16, device=meta)
    emb = torch.empty((B, rb.emb_channels), dtype=torch.float16, device=meta)
    ctx = dict(txt=torch.empty((r * B * 80, 1024), dtype=torch.float16, device=meta), img=torch.empty((r * B * 256, 1024), dtype=torch.float16, device=meta),
               n_img=256, per_frame=False)
    with torch.no_grad():
        kv = st.project_context(ctx)
        del rec.log[:]
        out = blk(x, emb, context={id(st): kv}, batch_size=B, cfg_repeat=r)
    assert out.shape == (r * B * T, hh, ww, st.in_channels) and isinstance(st, SpatialTransformer)
    return rec.log


# (T, h, w): 40 x 64 = level 0 of the 320 x 512 model; 3 frames are 7680 rows alone and 15360 in a pair (8192 rows: epilogue row statistics), 6
# frames 9.8 MB alone and 19.7 MB in a pair (16 MiB: the spatial GroupNorm fold); 16 x 40 x 64 and 25 x 72 x 128 are the shipped latents
ROUTE_GRID = [("inference_pvd_512.yaml", 3, 40, 64), ("inference_pvd_512.yaml", 6, 40, 64), ("inference_pvd_512.yaml", 16, 40, 64),
              ("inference_pvd_512.yaml", 25, 40, 64), ("inference_pvd_1024.yaml", 2, 72, 128), ("inference_pvd_1024.yaml", 25, 72, 128)]


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("yaml_name,T,h,w", ROUTE_GRID)
def test_batch_routes_do_not_depend_on_the_batch(monkeypatch, yaml_name, T, h, w, level):
    """Every batch-size-dependent decision of the host graph is made on per-video quantities: the launch sequence of a level-0 / level-1 block is
    the same for B = 1, B = 2 and the shared CFG prefix (cfg_repeat 2 / 3) - entry points, rows per unit, requested by-products.  (Bits of
    one route against another are the GPU suite's business: tests/test_batch_invariance_gpu.py.)"""
    one = _block_routes(monkeypatch, yaml_name, level, 1, T, h, w)
    assert _block_routes(monkeypatch, yaml_name, level, 2, T, h, w) == one, "B = 2 takes other routes than B = 1"
    for r in (2, 3):
        assert _block_routes(monkeypatch, yaml_name, level, 1, T, h, w, r=r) == one, f"the shared CFG prefix (r = {r}) takes other routes"


@pytest.mark.parametrize("yaml_name,T,h,w", [("inference_pvd_1024.yaml", 25, 72, 128), ("inference_pvd_512.yaml", 16, 40, 64)])
def test_batch_routes_at_the_shipped_latents_keep_the_fast_paths(monkeypatch, yaml_name, T, h, w):
    """At the benchmark's latents (B = 2: cond + uncond) level 0 keeps the spatial and temporal GroupNorm folds (proj_in as one
    vcx_gemm_units_f16 launch with per-frame / per-video weights) and LayerNorm statistics from the producers' epilogues."""
    log = _block_routes(monkeypatch, yaml_name, 0, 2, T, h, w)
    units = [e for e in log if e[0] == "gemm_units"]
    assert units == [("gemm_units", h * w, True), ("gemm_units", T * h * w, True)], units
    rowstats_linear = [e for e in log if e[0] == "gemm" and e[7]]
    assert len(rowstats_linear) == 2, rowstats_linear          # attn1's output projection, spatial and temporal
    assert not [e for e in log if e[0] == "row_stats"], "a LayerNorm statistics pass at level 0"


def _first_false(ok, lo, hi):
    """the smallest row count in (lo, hi] where the monotone predicate ok() turns false (ok(lo) true, ok(hi) false)"""
    assert ok(lo) and not ok(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return hi


def test_python_mirrors_of_the_extent_limit_flip_where_the_dispatcher_starts_rejecting():
    """The host graph asks ops.lnfold_ok / colstats_ok / rowstats_ok / conv_tail_ok / attention.fold_extent_ok before it sends a flagged
    call, and clip_batch caps a forward with its own copy of the limit.  Each mirror must turn false at exactly the row count where
    vcx_gemm_f16 starts to reject the same call (one row below: mirror true; at it: mirror false and the C dispatcher rejects, checked
    with fake pointers - the rejection comes before any launch), or a batched forward could send a flagged call across the line."""
    from tests.test_abi import EINVAL, FAKE, LIM, _gemm_rc
    from viewcrafter_amd import _lib as G, clip_batch, ops
    from viewcrafter_amd.lvdm.modules import attention as A
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "viewcrafter_amd", "csrc", "gemm.hip")).read()
    assert set(re.findall(r"lim = (0x[0-9A-Fa-f]+)ull", src)) == {"0xFFFF0000"} and LIM == clip_batch._LIM == 0xFFFF0000
    stats = dict(ln_stats=FAKE, ln_colsum=FAKE)
    # LNFOLD: operand extent through the row stride / output extent incl. the 256 rows past the end
    m = _first_false(lambda r: ops.lnfold_ok(r, 64, 64, lda=4096), 1000, 1 << 22)
    assert m == 524281 and _gemm_rc(M=m, N=64, K=64, lda=4096, ldc=64, flags=G.GEMM_LNFOLD, **stats)[0] == EINVAL
    m = _first_false(lambda r: ops.lnfold_ok(r, 960, 320), 460800, 1 << 24)          # q | k | v of level 0: the output (ldc = 960) goes first
    assert 2 * (m + 256) * 960 >= LIM > 2 * (m + 255) * 960 and _gemm_rc(M=m, N=960, K=320, lda=320, ldc=960, flags=G.GEMM_LNFOLD, **stats)[0] == EINVAL
    m = _first_false(lambda r: ops.lnfold_ok(8 * r, 320, 320, transposed=True), 1000, 1 << 22) * 8      # LNFOLD_T: the token rows are the W operand
    assert _gemm_rc(M=320, N=m, K=320, lda=320, ldw=320, ldc=m, flags=G.GEMM_LNFOLD_T | G.GEMM_BIAS_M, bias=FAKE, **stats)[0] == EINVAL
    assert ops.lnfold_ok(m - 8, 320, 320, transposed=True)
    # COLSTATS of a linear layer / a convolution (whole 64-row strips): output extent, then the input extent (in_rows)
    m = _first_false(lambda s: ops.colstats_ok(64 * s, 64, 320, 2560), 100, 1 << 20) * 64
    rc, msg = _gemm_rc(M=m, N=2560, K=320, lda=320, ldc=2560, flags=G.GEMM_COLSTATS, colstats=FAKE)
    assert 2 * (m + 256) * 2560 >= LIM > 2 * (m - 64 + 256) * 2560 and rc == EINVAL and b"COLSTATS" in msg
    n = _first_false(lambda k: ops.colstats_ok(k * 9216, 9216, 960, 320, in_rows=k * 9216), 50, 4000)      # frames of 72 x 128, 960 -> 320
    conv = dict(mode=1, in_h=72, in_w=128, out_h=72, out_w=128, cin=960, kh=3, kw=3, stride=1, pad_h=1, pad_w=1)
    rc, msg = _gemm_rc(M=n * 9216, N=320, K=9 * 960, lda=960, ldc=320, flags=G.GEMM_COLSTATS | G.GEMM_CONV_SLABK, colstats=FAKE, **conv)
    assert 2 * n * 9216 * 960 >= LIM > 2 * (n - 1) * 9216 * 960 and n > 175 and rc == EINVAL and b"COLSTATS" in msg      # 175 frames = 7 videos pass
    # K tail of that convolution (640 + 320 columns of the folded skip convolution)
    n = _first_false(lambda k: ops.conv_tail_ok(k * 9216, 960, 320, 9, (640, 320)), 50, 4000)
    rc, msg = _gemm_rc(M=n * 9216, N=320, K=9 * 960 + 960, lda=960, ldc=320, flags=G.GEMM_CONV_SLABK, tail_a0=FAKE, tail_lda0=640, tail_k0=640,
                       tail_a1=FAKE, tail_lda1=320, tail_k1=320, **conv)
    assert rc == EINVAL and b"K tail" in msg
    # ROWSTATS: extents of the call, and the statistics buffer (8 M) on its own
    rs = dict(N=320, K=320, rowstats=FAKE, rowstats_eps=1e-5, flags=G.GEMM_ROWSTATS)
    m = _first_false(lambda r: ops.rowstats_ok(r, 320, 320), 460800, 1 << 24)
    assert 2 * (m + 256) * 320 >= LIM > 2 * (m + 255) * 320 and _gemm_rc(M=m, lda=320, ldc=320, **rs)[0] == EINVAL
    m = _first_false(lambda r: ops.rowstats_ok(r, 320, 320, lda=4096), 460800, 1 << 24)
    assert 2 * ((m - 1) * 4096 + 320) >= LIM and _gemm_rc(M=m, lda=4096, ldc=320, **rs)[0] == EINVAL
    m = _first_false(lambda r: ops.rowstats_ok(r, 320, 320, lda=0, ldc=0), 460800, 1 << 30)
    assert m == LIM // 8 and _gemm_rc(M=m, lda=0, ldc=0, **rs)[0] == EINVAL
    # the one-launch vcx_gemm_units_f16 (GroupNorm folded into proj_in): its output bound is fold_extent_ok
    u = _first_false(lambda k: A.fold_extent_ok(k * 9216, 320), 50, 4000)
    assert 2 * (u * 9216 + 256) * 320 >= LIM > 2 * ((u - 1) * 9216 + 256) * 320 and not ops.rowstats_ok(u * 9216, 320, 320, unit_rows=9216)
    rc, msg = _gemm_rc(units=9216, M=u * 9216, lda=320, ldc=320, bias=FAKE, **dict(rs, flags=G.GEMM_ROWSTATS | G.GEMM_BIAS_N))
    assert rc == EINVAL and b"ROWSTATS" in msg          # (without the flag the call would leave the one-launch form and run unit by unit)

    # the clip-batch cap: the widest tensor of n videos (GEGLU output, 4 x 320 columns, and its 2560-column packed projection) stays
    # on the 32-bit routes, n + 1 does not - by the dispatcher's own arithmetic (out_ok) and by the mirrors
    class U:
        model_channels, channel_mult, attention_resolutions = 320, (1, 2, 4, 4), (4, 2, 1)
    V = 25 * 72 * 128
    n = clip_batch.max_videos_per_forward(U, 25, 72, 128)
    assert n == 7 and 2 * (n * V + 256) * 1280 < LIM <= 2 * ((n + 1) * V + 256) * 1280
    assert ops.lnfold_ok(n * V, 1280, 320, ldc=1280) and not ops.lnfold_ok((n + 1) * V, 1280, 320, ldc=1280)
    assert ops.colstats_ok(n * V, V, 1280, 320) and not ops.colstats_ok((n + 1) * V, V, 1280, 320)
    rc, msg = _gemm_rc(M=(n + 1) * V, N=320, K=1280, lda=1280, ldc=320, flags=G.GEMM_COLSTATS, colstats=FAKE)       # the layer behind it, reading 8 videos
    assert rc == EINVAL and b"COLSTATS" in msg

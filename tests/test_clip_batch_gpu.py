"""Several clips in ONE denoising loop per GPU (VCX_CLIP_BATCH, viewcrafter_amd/clip_batch.py) on the MI355X.

The bar is bit-identity: every clip's video batched k at a time equals, bit for bit, the video the plain loop (parallel.run_sharded with
lanes=1, clip i after `torch.manual_seed(seed + i)`, clip 0 continuing the current state) gives it, and the CPU and CUDA generators are
left in the same state - on the tiny hybrid model (CFG and multi-condition guidance, warm and cold), at full width with synthetic
weights (320 x 512 x 25 and 576 x 1024 x 25, where a requested k = 4 is capped to the 3 clips that fit the GEMM engine's 32-bit
extents), and through `inference.py --renderings a.pt,b.pt,c.pt`."""
import os
import subprocess
import sys

import pytest
import torch

from oracle.weights import synth_input
from tests.util import SCHEDULE_BUFFERS, load_synth, write_tiny_entry_files

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1234


@pytest.fixture(scope="module")
def igs_model():
    from tests.tiny_config import CLIP_TINY, CLIP_TINY_CFG, igs_model_params
    from viewcrafter_amd.config import Config
    from viewcrafter_amd.lvdm.modules.encoders import condition as cond
    from viewcrafter_amd.utils.diffusion_utils import instantiate_from_config
    cond.CLIP_CONFIGS[CLIP_TINY] = CLIP_TINY_CFG
    R = "lvdm.modules.encoders."
    params = Config.wrap(igs_model_params("lvdm.modules.networks.openaimodel3d.UNetModel", "lvdm.models.autoencoder.AutoencoderKL",
                                          R + "condition.FrozenOpenCLIPEmbedder", R + "condition.FrozenOpenCLIPImageEmbedderV2",
                                          R + "resampler.Resampler"))
    m = instantiate_from_config(Config(target="lvdm.models.ddpm3d.VIPLatentDiffusion", params=params)).eval()
    load_synth(m, skip=SCHEDULE_BUFFERS)
    return m.to(DEV)


def _plain_and_batched(model, clips, noise_shape, ks, steps=4, multicond=False, cold=False):
    """{'plain': (videos, cuda state, cpu state), k: (...)} - the plain loop once, then batched at every k of `ks`."""
    from viewcrafter_amd import clip_batch, parallel
    from viewcrafter_amd.utils.diffusion_utils import image_guided_synthesis, image_guided_synthesis_clips
    kw = dict(n_samples=1, ddim_steps=steps, ddim_eta=1.0, unconditional_guidance_scale=7.5, cfg_img=3.0 if multicond else None,
              fs=10, text_input=False, multiple_cond_cfg=multicond, timestep_spacing="uniform_trailing", guidance_rescale=0.7,
              condition_index=[0])

    def one(videos, index):
        if index > 0:
            torch.manual_seed(SEED + index)
        with torch.no_grad():
            return image_guided_synthesis(model, [""], videos, noise_shape, **kw)

    def group(videos, indices):
        streams = clip_batch.ClipStreams([None if i == 0 else SEED + i for i in indices])
        with torch.no_grad():
            outs = image_guided_synthesis_clips(model, [""], videos, noise_shape, streams=streams, **kw)
        streams.finish()
        return outs

    def state(res):
        torch.cuda.synchronize()
        return [res[i].clone() for i in range(len(clips))], torch.cuda.get_rng_state().clone(), torch.random.get_rng_state().clone()
    got = {}
    torch.manual_seed(5)
    got["plain"] = state(parallel.run_sharded(one, clips, gather=False, lanes=1))
    for k in ks:
        if cold:
            parallel.drop_packed_copies(model)
        torch.manual_seed(5)
        got[k] = state(parallel.run_sharded_batched(group, clips, k, gather=False))
    return got


def _check(got, n):
    want = got["plain"]
    assert all(torch.isfinite(v).all() for v in want[0])
    for i in range(n - 1):
        assert not torch.equal(want[0][i], want[0][i + 1]), "distinct clips must give distinct videos"
    for k, res in got.items():
        if k == "plain":
            continue
        for i in range(n):
            assert torch.equal(res[0][i], want[0][i]), (f"k = {k}: clip {i} differs from the plain loop in "
                                                        f"{int((res[0][i] != want[0][i]).sum())} elements")
        assert torch.equal(res[1], want[1]) and torch.equal(res[2], want[2]), f"k = {k}: generators not left as the plain loop leaves them"


def _tiny_clips(n, tag):
    from tests.tiny_config import IGS_H, IGS_T, IGS_W
    clips = [torch.tanh(synth_input(f"{tag}{i}", (1, 3, IGS_T, IGS_H, IGS_W))).to(DEV) for i in range(n)]
    return clips, [1, 4, IGS_T, IGS_H // 8, IGS_W // 8]


@pytest.mark.parametrize("n,ks", [(3, (2, 3)), (5, (2,))])
def test_batched_clips_equal_the_plain_loop_cfg(igs_model, n, ks):
    clips, noise_shape = _tiny_clips(n, "cbatch_videos")
    _check(_plain_and_batched(igs_model, clips, noise_shape, ks), n)


def test_batched_clips_equal_the_plain_loop_multicond(igs_model):
    clips, noise_shape = _tiny_clips(3, "cbatch_mc_videos")
    _check(_plain_and_batched(igs_model, clips, noise_shape, (2, 3), multicond=True), 3)


def test_batched_clips_on_a_cold_model_equal_the_plain_loop(igs_model):
    """Every kernel-layout pack dropped before the batched run: the packs it builds on the fly give the same bits."""
    clips, noise_shape = _tiny_clips(3, "cbatch_cold_videos")
    _check(_plain_and_batched(igs_model, clips, noise_shape, (2,), cold=True), 3)


def test_driver_refuses_clip_batch_beside_two_streams(igs_model, monkeypatch):
    import types
    import viewcrafter
    vc = viewcrafter.ViewCrafter.__new__(viewcrafter.ViewCrafter)
    vc.__dict__.update(opts=types.SimpleNamespace(seed=SEED), _ref=None, diffusion=igs_model, device=DEV)
    monkeypatch.setenv("VCX_CLIP_BATCH", "2")
    monkeypatch.setenv("VCX_CLIPS_PER_GPU", "2")
    clips, _ = _tiny_clips(2, "cbatch_refuse")
    with pytest.raises(ValueError, match="cannot be combined"):
        vc.run_diffusion_many(clips)


# ------------------------------------------------------------------------------------------------------ full width, synthetic weights
def _full_model(yaml_name, seed):
    from viewcrafter_amd.builder import build_diffusion_model, randomize_parameters
    m = build_diffusion_model(os.path.join(ROOT, "configs", yaml_name), device=DEV, conditioners="config")
    randomize_parameters(m, seed=seed)
    return m.eval()


def _full_clips(n, T, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(T, H, W, 3, generator=g) * 2. - 1.).permute(3, 0, 1, 2).unsqueeze(0).to(DEV) for _ in range(n)]


def test_full_width_512_two_clips_batched_equal_sequential():
    m = _full_model("inference_pvd_512.yaml", seed=21)
    T, H, W = 25, 320, 512
    got = _plain_and_batched(m, _full_clips(2, T, H, W, 31), [1, 4, T, H // 8, W // 8], (2,), steps=2)
    _check(got, 2)
    del m
    torch.cuda.empty_cache()


def test_full_width_1024_batched_and_capped_at_the_extent_limit_equal_sequential():
    """576 x 1024 x 25 with CFG: k = 2, and a requested k = 4 capped to 3 (7 videos of 590 MB feed-forward hidden state fit the 32-bit
    extents, 8 would not) - groups of 3 + 1 clips, bit-identical to the plain loop."""
    from viewcrafter_amd import clip_batch
    m = _full_model("inference_pvd_1024.yaml", seed=22)
    T, H, W = 25, 576, 1024
    noise_shape = [1, 4, T, H // 8, W // 8]
    cap = clip_batch.max_clips_per_forward(m.model.diffusion_model, noise_shape, clip_batch.guidance_copies(7.5))
    assert cap == 3
    got = _plain_and_batched(m, _full_clips(4, T, H, W, 32), noise_shape, (2, min(4, cap)), steps=2)
    _check(got, 4)
    del m
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------ command line
def test_inference_cli_with_clip_batch_equals_the_plain_run(tmp_path):
    from tests.tiny_config import IGS_H, IGS_T, IGS_W
    ypath, cpath, rpath, (T, H, W) = write_tiny_entry_files(tmp_path)
    paths = [rpath]
    for i in (1, 2):
        g = torch.Generator().manual_seed(50 + i)
        paths.append(os.path.join(str(tmp_path), f"renders{i}.pt"))
        torch.save(torch.rand(IGS_T, IGS_H, IGS_W, 3, generator=g), paths[-1])
    outs = {}
    for tag, k in (("plain", None), ("batched", "2")):
        env = {key: v for key, v in os.environ.items() if key not in ("VCX_CLIP_BATCH", "VCX_CLIPS_PER_GPU")}
        if k is not None:
            env["VCX_CLIP_BATCH"] = k
        out_dir = str(tmp_path / f"out_{tag}")
        cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "--renderings", ",".join(paths), "--config", ypath, "--ckpt_path",
               cpath, "--out_dir", out_dir, "--exp_name", "e", "--device", "cuda:0", "--ddim_steps", "4", "--video_length", str(T),
               "--height", str(H), "--width", str(W), "--prompt", "", "--seed", "123"]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        outs[tag] = [torch.load(os.path.join(out_dir, "e", f"diffusion{i}.pt")) for i in range(3)]
    for i in range(3):
        assert torch.equal(outs["plain"][i], outs["batched"][i]), f"diffusion{i}.pt differs with VCX_CLIP_BATCH=2"
    assert not torch.equal(outs["plain"][0], outs["plain"][1])

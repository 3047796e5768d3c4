"""Several clips in one denoising loop (VCX_CLIP_BATCH, viewcrafter_amd/clip_batch.py), the host side: per-clip generator contexts
against a plain loop of `manual_seed(seed + i)` draws (CPU generator), the 4 GiB cap per workload, the grouping of a rank's clips and the
refusal of VCX_CLIPS_PER_GPU beside it."""
import os
import types

import pytest
import torch

from viewcrafter_amd import clip_batch, parallel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 123
STEPS = 3
LAT = (1, 4, 3, 5, 6)          # one clip's x_T / per-step noise
POST = (3, 4, 5, 6)            # one clip's posterior noise of the VAE encode (CPU in the product as well)


def _plain(n, continue_first):
    """What viewcrafter.py::run_diffusion_many's plain loop draws: per clip the conditioning's draw, x_T, one noise per step."""
    out = []
    for i in range(n):
        if i > 0 or not continue_first:
            torch.manual_seed(SEED + i)
        out.append([torch.randn(POST), torch.randn(LAT)] + [torch.randn(LAT) for _ in range(STEPS)])
    return out, torch.random.get_rng_state()


def _batched(n, k, continue_first):
    out = [None] * n
    for group in clip_batch.groups(range(n), k):
        streams = clip_batch.ClipStreams([None if (i == 0 and continue_first) else SEED + i for i in group], cuda=False)
        posts = []
        for j in range(len(group)):
            with streams.clip(j):
                posts.append(torch.randn(POST))
        shape = (len(group) * LAT[0],) + LAT[1:]
        draws = [streams.randn(shape)] + [streams(shape) for _ in range(STEPS)]
        for j, i in enumerate(group):
            out[i] = [posts[j]] + [d[j:j + 1] for d in draws]
        streams.finish()
    return out, torch.random.get_rng_state()


@pytest.mark.parametrize("n,k", [(3, 2), (3, 3), (5, 2), (4, 4), (2, 1)])
@pytest.mark.parametrize("continue_first", [True, False])
def test_clip_contexts_equal_the_plain_loop_of_seeded_draws(n, k, continue_first):
    torch.manual_seed(77)
    want, want_state = _plain(n, continue_first)
    torch.manual_seed(77)
    got, got_state = _batched(n, k, continue_first)
    for i in range(n):
        assert all(torch.equal(a, b) for a, b in zip(want[i], got[i])), f"clip {i} draws differ from its plain-loop stream"
    assert torch.equal(want_state, got_state), "the global CPU generator is not left as after the plain loop"
    assert not torch.equal(got[0][1], got[1][1])


def test_draws_outside_a_clip_context_do_not_disturb_the_clips():
    torch.manual_seed(5)
    streams = clip_batch.ClipStreams([SEED, SEED + 1], cuda=False)
    before = torch.random.get_rng_state()
    with streams.clip(0):
        a = torch.randn(4)
    assert torch.equal(torch.random.get_rng_state(), before)          # the caller's state comes back
    torch.randn(100)
    with streams.clip(0):
        b = torch.randn(4)
    torch.manual_seed(SEED)
    assert torch.equal(torch.cat([a, b]), torch.randn(8))
    with pytest.raises(ValueError):
        streams.randn((3, 2))


def test_groups_of_a_ranks_clips():
    assert clip_batch.groups([0, 1, 2, 3, 4], 2) == [[0, 1], [2, 3], [4]]
    assert clip_batch.groups([1, 3, 5], 3) == [[1, 3, 5]]
    assert clip_batch.groups([], 2) == []


def test_run_sharded_batched_groups_in_order_and_keeps_indices():
    seen = []

    def fn(items, indices):
        seen.append(list(indices))
        return [x * 10 for x in items]
    out = parallel.run_sharded_batched(fn, [1, 2, 3, 4, 5], 2)
    assert out == [10, 20, 30, 40, 50] and seen == [[0, 1], [2, 3], [4]]


def test_clip_batch_env_default_and_refusal_beside_two_streams():
    assert clip_batch.clip_batch_from_env({}) == 1
    assert clip_batch.clip_batch_from_env({"VCX_CLIP_BATCH": "3"}) == 3
    assert clip_batch.clip_batch_from_env({"VCX_CLIP_BATCH": "1", "VCX_CLIPS_PER_GPU": "2"}) == 1
    for bad in ("0", "-1", "two"):
        with pytest.raises(ValueError):
            clip_batch.clip_batch_from_env({"VCX_CLIP_BATCH": bad})
    with pytest.raises(ValueError, match="cannot be combined"):
        clip_batch.clip_batch_from_env({"VCX_CLIP_BATCH": "2", "VCX_CLIPS_PER_GPU": "2"})


def test_driver_refuses_clip_batch_with_two_streams(monkeypatch):
    import viewcrafter
    vc = viewcrafter.ViewCrafter.__new__(viewcrafter.ViewCrafter)
    vc.__dict__.update(opts=types.SimpleNamespace(seed=SEED), _ref=None)
    monkeypatch.setenv("VCX_CLIP_BATCH", "2")
    monkeypatch.setenv("VCX_CLIPS_PER_GPU", "2")
    with pytest.raises(ValueError, match="VCX_CLIP_BATCH=2 and VCX_CLIPS_PER_GPU=2 cannot be combined"):
        vc.run_diffusion_many([torch.zeros(1), torch.zeros(1)])


def _unet_of(yaml_name):
    from viewcrafter_amd.config import load_yaml
    p = load_yaml(os.path.join(ROOT, "configs", yaml_name))["model"]["params"]["unet_config"]["params"]
    return types.SimpleNamespace(model_channels=p["model_channels"], channel_mult=p["channel_mult"],
                                 attention_resolutions=p["attention_resolutions"])


def test_extent_cap_per_workload():
    """Level 0 of the 576 x 1024 model holds the widest tensor: 25 x 72 x 128 rows x 1280 fp16 columns = 590 MB per video, 7 videos below
    the engine's 32-bit limit - k <= 3 with CFG, 2 with multi-condition guidance, 7 without guidance; 8 videos would cross it."""
    u = _unet_of("inference_pvd_1024.yaml")
    assert clip_batch.max_videos_per_forward(u, 25, 72, 128) == 7
    lim = 0xFFFF0000
    rows, width = 25 * 72 * 128, 4 * 320
    assert 2 * (7 * rows + 256) * width < lim <= 2 * (8 * rows + 256) * width
    shape = [1, 4, 25, 72, 128]
    assert [clip_batch.max_clips_per_forward(u, shape, r) for r in (1, 2, 3)] == [7, 3, 2]
    assert clip_batch.max_clips_per_forward(u, [1, 4, 16, 72, 128], 2) == 5
    u512 = _unet_of("inference_pvd_512.yaml")
    assert clip_batch.max_videos_per_forward(u512, 25, 40, 64) == 26
    assert clip_batch.max_clips_per_forward(u512, [1, 4, 25, 40, 64], 2) == 13
    assert clip_batch.guidance_copies(1.0) == 1 and clip_batch.guidance_copies(7.5) == 2
    assert clip_batch.guidance_copies(7.5, True, 3.0) == 3 and clip_batch.guidance_copies(7.5, True, 1.0) == 2

"""Several clips in ONE denoising loop per GPU (VCX_CLIP_BATCH=k; default 1 = one clip after the other).

A rank that owns more clips than it has GPUs can stack k of them on the batch axis and run one DDIM loop over B = k (k x 2 videos per
UNet forward with CFG, k x 3 with multi-condition guidance).  Every route decision of the host graph is made per video and the kernels'
bits do not depend on the batch (tests/test_batch_invariance_gpu.py), so a clip's video only depends on its own random draws.  Those are
kept here: each clip has its own saved (CPU, CUDA) generator state, and every draw of clip i - the posterior noise of its VAE encode
(CPU), its x_T and one Gaussian per DDIM step (CUDA) - is made inside clip i's context, in the order the plain loop makes them
(viewcrafter.py::run_diffusion_many: clip i after `torch.manual_seed(seed + i)`).  The videos are bit-identical to the plain loop's.

Limit (`max_clips_per_forward`): the tiled GEMM engine addresses every operand with 32-bit byte offsets (csrc/gemm_dma.hip, gemm.hip
`dma_ok`).  The largest tensor of a forward is the feed-forward hidden state of the first UNet level (4 x model_channels wide, fp16); at
576 x 1024 x 25 that is 590 MB per video, so at most 7 videos fit one call: k <= 3 with CFG, k <= 2 with multi-condition guidance.  A
larger VCX_CLIP_BATCH is CAPPED to that (the groups get smaller), never split inside a forward, so no call leaves its route.

Measured sign (profiles/r07_clip_batch_ab.md) and the k limits are in README.md / DESIGN.md."""
import contextlib
import os

import torch

_LIM = 0xFFFF0000          # the engine's extent limit (csrc/gemm.hip `lim`): byte offsets up to 256 rows past the end stay below it


def clip_batch_from_env(environ=None):
    """VCX_CLIP_BATCH as an int >= 1 (default 1).  Refuses VCX_CLIPS_PER_GPU > 1 beside it: batching and the two-stream lanes
    (interleave.py) are not combined."""
    env = os.environ if environ is None else environ
    raw = env.get("VCX_CLIP_BATCH", "1").strip() or "1"
    try:
        k = int(raw)
    except ValueError:
        raise ValueError(f"VCX_CLIP_BATCH must be a positive integer, got {raw!r}") from None
    if k < 1:
        raise ValueError(f"VCX_CLIP_BATCH must be a positive integer, got {raw!r}")
    try:
        lanes = int(env.get("VCX_CLIPS_PER_GPU", "1"))
    except ValueError:
        lanes = 1
    if k > 1 and lanes > 1:
        raise ValueError(f"VCX_CLIP_BATCH={k} and VCX_CLIPS_PER_GPU={lanes} cannot be combined: batch the clips of a rank into one "
                         "forward (VCX_CLIP_BATCH) OR run them on two HIP streams (VCX_CLIPS_PER_GPU), not both")
    return k


def guidance_copies(unconditional_guidance_scale, multiple_cond_cfg=False, cfg_img=None):
    """Videos per clip in one UNet forward: 1 without guidance, 2 with CFG, 3 with multi-condition CFG (image_guided_synthesis)."""
    if unconditional_guidance_scale == 1.0:
        return 1
    return 3 if (multiple_cond_cfg and cfg_img != 1.0) else 2


def max_videos_per_forward(unet, frames, h, w):
    """How many videos of `frames` x h x w latents one UNet forward can take before a tensor's byte offsets reach the tiled engine's 32-bit
    limit.  The widest activation per row is the feed-forward hidden state (4 x channels, GEGLU output, fp16) of a level with attention;
    levels without attention still hold 3 x channels (the concatenated skip input of the decoder).  Per level: the largest n with
    2 B x (n x rows + 256) x width < limit (the engine's output descriptor also addresses 256 rows past the end)."""
    mc, mult = unet.model_channels, list(unet.channel_mult)
    attn = set(unet.attention_resolutions or ())
    n = None
    for lvl, m in enumerate(mult):
        ds = 2 ** lvl
        rows = frames * ((h + ds - 1) // ds) * ((w + ds - 1) // ds)
        width = (4 if ds in attn else 3) * mc * m
        n_lvl = ((_LIM - 1) // (2 * width) - 256) // rows
        n = n_lvl if n is None else min(n, n_lvl)
    return max(1, n)


def max_clips_per_forward(unet, noise_shape, copies):
    """The largest k that `max_videos_per_forward` allows for clips of noise_shape = [b, C, T, h, w] with `copies` videos each (>= 1)."""
    b, _, t, h, w = noise_shape
    return max(1, max_videos_per_forward(unet, t, h, w) // (copies * b))


def groups(indices, k):
    """A rank's owned clip indices, k at a time (the last group may be smaller)."""
    indices = list(indices)
    return [indices[i:i + k] for i in range(0, len(indices), k)]


def _state(cuda):
    return torch.random.get_rng_state(), (torch.cuda.get_rng_state() if cuda else None)


def _restore(state, cuda):
    torch.random.set_rng_state(state[0])
    if cuda and state[1] is not None:
        torch.cuda.set_rng_state(state[1])


class ClipStreams:
    """One (CPU, CUDA) generator state per clip.  seeds[i]: an int gives the state `torch.manual_seed(seed)` leaves; None continues the
    current global state (clip 0 of a one-process run, as in the plain loop).  `with streams.clip(i):` makes the global generators clip
    i's for the draws inside and restores the caller's afterwards; `finish()` leaves them as the plain loop would (after the last clip)."""

    def __init__(self, seeds, cuda=None):
        self.cuda = torch.cuda.is_available() if cuda is None else bool(cuda)
        self.seeds = list(seeds)
        outer = _state(self.cuda)
        self.states = []
        for s in self.seeds:
            if s is None:
                self.states.append(outer)
            else:
                torch.manual_seed(int(s))
                self.states.append(_state(self.cuda))
                _restore(outer, self.cuda)

    def __len__(self):
        return len(self.states)

    @contextlib.contextmanager
    def clip(self, i):
        outer = _state(self.cuda)
        _restore(self.states[i], self.cuda)
        try:
            yield
        finally:
            self.states[i] = _state(self.cuda)
            _restore(outer, self.cuda)

    def randn(self, shape, device=None):
        """torch.randn(shape) with the batch axis split evenly over the clips, each part drawn in its clip's context (the sampler's noise
        source: x_T and the per-step noise, ddim.py)."""
        n = len(self.states)
        if shape[0] % n:
            raise ValueError(f"batch {shape[0]} is not a whole number of rows for {n} clips")
        per = (shape[0] // n,) + tuple(shape[1:])
        parts = []
        for i in range(n):
            with self.clip(i):
                parts.append(torch.randn(per, device=device))
        return torch.cat(parts, 0)

    def __call__(self, shape, device=None):
        return self.randn(shape, device)

    def finish(self):
        """Global generators as after the plain loop: the last clip's manual_seed (every CUDA device), then its state after its draws."""
        if self.seeds and self.seeds[-1] is not None:
            torch.manual_seed(int(self.seeds[-1]))
        _restore(self.states[-1], self.cuda)

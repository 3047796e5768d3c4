"""Opt-in feature cache (VCX_FEATURE_CACHE=N, VCX_FEATURE_CACHE_DEPTH=d): shallow UNet forwards between full denoising steps.

The deep features of the UNet change slowly from one denoising step to the next (DeepCache, Ma et al., CVPR 2024), so with interval N
only every N-th step runs the whole UNet.  A FULL forward is today's forward, except that the concat target which
output_blocks[L-2-d] writes lives in storage owned by the UNet that survives the forward.  A SHALLOW forward runs input_blocks[0..d]
(and init_attn), skips everything up to and including output_blocks[L-2-d], and runs output_blocks[L-1-d ..] and the output head on top
of that kept target, with freshly computed skips.  Nothing else is approximated: every layer that runs, runs on the current x, t, fs and
context.  Quality with a real checkpoint is unmeasured - the switch is off by default.

This module holds what the samplers and the UNet share: the schedule (one pure function), the parsing of the two variables (read when a
sample() call starts, like VCX_SAMPLER) and the small per-call object that carries the mode of the next forward, the depth, the slot and
the validity of what the slot holds.
"""
import os

from .interleave import current_lane

MODES = ("full", "shallow")


def feature_cache_plan(total_steps, interval):
    """[step i is a full forward] for the loop positions i = 0 .. total_steps-1 in the order the sampler walks (i = 0 is the noisiest
    step): full iff i % interval == 0.  interval < 2 = every step full."""
    n = max(int(interval), 1)
    return [i % n == 0 for i in range(int(total_steps))]


def feature_cache_interval():
    """VCX_FEATURE_CACHE: unset, empty, 0 or 1 -> 0 (off); N >= 2 -> N; anything else is an error."""
    raw = os.environ.get("VCX_FEATURE_CACHE", "").strip()
    if raw == "":
        return 0
    try:
        n = int(raw)
    except ValueError:
        n = -1
    if n < 0:
        raise ValueError(f"VCX_FEATURE_CACHE={os.environ['VCX_FEATURE_CACHE']!r}: expected an interval N >= 2 (every N-th step is a full UNet forward), "
                         f"or 0 / 1 / unset for no cache")
    return n if n >= 2 else 0


def feature_cache_depth(n_blocks=None):
    """VCX_FEATURE_CACHE_DEPTH: d input blocks beyond the first (and as many output blocks beyond the last) run on a shallow step;
    default 0.  n_blocks = len(input_blocks) of the UNet, when known: the range is 0 .. n_blocks - 2."""
    raw = os.environ.get("VCX_FEATURE_CACHE_DEPTH", "").strip()
    hi = None if n_blocks is None else n_blocks - 2
    rng = "an integer >= 0" if hi is None else f"an integer in 0 .. {hi}"
    try:
        d = int(raw) if raw else 0
    except ValueError:
        d = -1
    if d < 0 or (hi is not None and d > hi):
        raise ValueError(f"VCX_FEATURE_CACHE_DEPTH={raw!r}: expected {rng}")
    return d


class FeatureCache:
    """What UNetModel.forward(feature_cache=...) takes: `mode` of the next forward ("full" / "shallow"), `depth`, and the slot - one stream
    of consecutive evaluations of the same thing: (lane of VCX_CLIPS_PER_GPU, position of the evaluation where a step evaluates its
    conditionings one after the other).  The storage belongs to the UNet; this object, local to one sample() call, knows which slots a full
    forward OF THIS CALL has filled and with what shapes, so a shallow forward can never read what another call left behind."""
    __slots__ = ("mode", "depth", "lane", "position", "filled")

    def __init__(self, depth=0, lane=None):
        self.mode, self.depth, self.position = "full", int(depth), 0
        self.lane = current_lane() if lane is None else lane
        self.filled = {}            # slot -> (input shapes, cfg_repeat, depth) of the full forward that filled it

    @property
    def slot(self):
        return (self.lane, self.position)

    def set_mode(self, mode):
        if mode not in MODES:
            raise ValueError(f"feature cache mode {mode!r}: expected one of {MODES}")
        self.mode = mode

    def check(self, shapes, cfg_repeat):
        """Called by the UNet ahead of a shallow forward: raises unless a full forward of this call filled the slot at these shapes."""
        got = self.filled.get(self.slot)
        if got is None:
            raise RuntimeError(f"feature cache: shallow forward in slot {self.slot}, which no full forward of this sample() call has filled")
        if got[0] != shapes:
            raise RuntimeError(f"feature cache: shallow forward with input shapes {shapes} in slot {self.slot}, filled at {got[0]}")
        if got[1] != cfg_repeat:
            raise RuntimeError(f"feature cache: shallow forward with cfg_repeat {cfg_repeat} in slot {self.slot}, filled at cfg_repeat {got[1]}")
        if got[2] != self.depth:
            raise RuntimeError(f"feature cache: shallow forward at depth {self.depth} in slot {self.slot}, filled at depth {got[2]}")

    def mark_filled(self, shapes, cfg_repeat):
        self.filled[self.slot] = (shapes, cfg_repeat, self.depth)


def from_env(denoiser=None):
    """(FeatureCache, interval) for one sample() call, or (None, 0) with the switch off.  `denoiser`: the UNet, for the depth's range."""
    n = feature_cache_interval()
    if n == 0:
        return None, 0
    blocks = getattr(denoiser, "input_blocks", None)
    return FeatureCache(depth=feature_cache_depth(None if blocks is None else len(blocks))), n

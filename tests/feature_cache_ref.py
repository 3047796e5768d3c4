"""fp32 reference of the feature cache (viewcrafter_amd/feature_cache.py), composed from the oracle's own pieces - the yardstick of
tests/test_feature_cache_cpu.py and tests/test_feature_cache_gpu.py.

A FULL forward is oracle.lvdm_oracle.unet_forward; its `taps` give the output of output_blocks[L-2-d], the feature a shallow forward
goes on from.  A SHALLOW forward runs input_blocks[0..d] (init_attn behind block 0), then output_blocks[L-1-d ..] on [kept | skip] and the
output head - the same layer functions on a subset of the layers.  CachedDenoiser is the stateful apply_model that follows
feature_cache_plan, one kept feature per evaluation of a step, for oracle.ddim_sample and tests/dpmpp_ref.loop.
"""
import torch
import torch.nn.functional as F

from oracle import lvdm_oracle as O
from viewcrafter_amd.feature_cache import feature_cache_plan


def kept_name(hp, depth):
    return f"output_blocks.{len(O.unet_layout(hp)[2]) - 2 - depth}"


def full_forward(sd, hp, x, timesteps, context, fs, depth):
    """(unet_forward's output, the feature that a shallow forward at `depth` goes on from)"""
    taps = {}
    y = O.unet_forward(sd, hp, x, timesteps, context, fs, taps=taps)
    return y, taps[kept_name(hp, depth)]


def shallow_forward(sd, hp, x, timesteps, context, fs, kept, depth):
    """unet_forward (openaimodel3d.py:548-603) without input_blocks[d+1 ..], the middle block and output_blocks[.. L-2-d]: `kept` stands
    where their result would."""
    b, _, t, _, _ = x.shape
    mc = hp["model_channels"]
    emb = O._lin(sd, "time_embed.2", F.silu(O._lin(sd, "time_embed.0", O.timestep_embedding(timesteps, mc))))
    L = context.shape[1]
    if L == 77 + t * 16:
        context = torch.cat([context[:, :77].repeat_interleave(t, dim=0), context[:, 77:].reshape(b * t, 16, -1)], dim=1)
    else:
        context = context.repeat_interleave(t, dim=0)
    emb = emb.repeat_interleave(t, dim=0)
    h = x.permute(0, 2, 1, 3, 4).reshape(b * t, x.shape[1], x.shape[3], x.shape[4])
    if hp.get("fs_condition", False):
        if fs is None:
            fs = torch.full((b,), hp.get("default_fs", 4), dtype=torch.long, device=x.device)
        fe = O._lin(sd, "fps_embedding.2", F.silu(O._lin(sd, "fps_embedding.0", O.timestep_embedding(fs, mc))))
        emb = emb + fe.repeat_interleave(t, dim=0)
    inputs, _, outputs = O.unet_layout(hp)
    n_out = len(outputs)
    assert 0 <= depth <= n_out - 2
    causal = bool(hp.get("use_causal_attention", False))
    hs = []
    for i in range(depth + 1):
        h = O._run_layers(sd, f"input_blocks.{i}", inputs[i], h, emb, context, b, causal)
        if i == 0 and hp.get("addition_attention", False):
            n, c, hh, ww = h.shape
            h5 = O.temporal_transformer(sd, "init_attn.0", h.view(b, t, c, hh, ww).permute(0, 2, 1, 3, 4), 8)
            h = h5.permute(0, 2, 1, 3, 4).reshape(n, c, hh, ww)
        hs.append(h)
    h = kept
    for j in range(n_out - 1 - depth, n_out):
        h = torch.cat([h, hs.pop()], dim=1)
        h = O._run_layers(sd, f"output_blocks.{j}", outputs[j], h, emb, context, b, causal)
    y = F.conv2d(F.silu(O._gn(sd, "out.0", h, 1e-5)), sd["out.2.weight"], sd["out.2.bias"], padding=1)
    return y.view(b, t, -1, y.shape[2], y.shape[3]).permute(0, 2, 1, 3, 4)


class CachedDenoiser:
    """apply_model(x, t, c) for oracle.ddim_sample: `evals` evaluations per step in a fixed order, each with its own kept feature; step i
    (counted in calls) is full where feature_cache_plan says so.  prepare(x, c) -> (UNet input, context) is the DiffusionWrapper."""

    def __init__(self, sd, hp, fs, total_steps, interval, depth, evals, prepare):
        self.sd, self.hp, self.fs, self.depth, self.evals, self.prepare = sd, hp, fs, depth, evals, prepare
        self.plan = feature_cache_plan(total_steps, interval)
        self.calls, self.kept, self.modes = 0, {}, []

    def __call__(self, x, t, c):
        step, pos = divmod(self.calls, self.evals)
        self.calls += 1
        xin, ctx = self.prepare(x.float(), c)
        if self.plan[step]:
            y, self.kept[pos] = full_forward(self.sd, self.hp, xin, t, ctx, self.fs, self.depth)
        else:
            y = shallow_forward(self.sd, self.hp, xin, t, ctx, self.fs, self.kept[pos], self.depth)
        if pos == 0:
            self.modes.append("full" if self.plan[step] else "shallow")
        return y

"""fp32 reference of the spatial self-attention over 2x2-pooled keys and values (VCX_SATTN_KV_POOL, viewcrafter_amd/lvdm/modules/attention.py),
composed from the oracle's own pieces - the yardstick of tests/test_sattn_kv_pool_cpu.py and tests/test_sattn_kv_pool_gpu.py.

spatial_transformer is oracle.lvdm_oracle.spatial_transformer with one change: where kv_pool_plan (the product's own, pure decision) pools
a frame's H x W tokens, attn1 of every block takes to_k and to_v of the POOLED normalised tokens - the mean over each 2x2 window of
norm1(x), or its row (2y, 2x) - while to_q sees every token.  Everything else (the cross-attention, the feed-forward, proj_in / proj_out,
the residuals) is the oracle's function, called as the oracle calls it.  unet_forward is the oracle's with that transformer in place of
its own."""
import contextlib

import torch.nn.functional as F

from oracle import lvdm_oracle as O
from viewcrafter_amd.lvdm.modules import attention as A


def pool_tokens(t, H, W, mode):
    """t [n, H W, C] -> [n, (H/2) (W/2), C]: the mean of each 2x2 window, or its row (2y, 2x)"""
    n, _, C = t.shape
    g = t.view(n, H, W, C)
    if mode == "nearest":
        return g[:, ::2, ::2].reshape(n, -1, C)
    return F.avg_pool2d(g.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).reshape(n, -1, C)


def pooled_self_attention(sd, p, xn, heads, H, W, mode):
    """oracle.cross_attention with context None, except that to_k / to_v read pool_tokens(xn)"""
    scale = (sd[p + ".to_q.weight"].shape[0] // heads) ** -0.5
    kv = pool_tokens(xn, H, W, mode)
    q, k, v = O._lin(sd, p + ".to_q", xn), O._lin(sd, p + ".to_k", kv), O._lin(sd, p + ".to_v", kv)
    out = O._unheads(O._sdpa(O._heads(q, heads), O._heads(k, heads), O._heads(v, heads), scale), heads)
    return O._lin(sd, p + ".to_out.0", out)


def transformer_block(sd, p, x, context, heads, H, W, mode):
    """oracle.transformer_block (image_cross_attention) with the pooled attn1"""
    x = pooled_self_attention(sd, p + ".attn1", O._ln(sd, p + ".norm1", x), heads, H, W, mode) + x
    x = O.cross_attention(sd, p + ".attn2", O._ln(sd, p + ".norm2", x), context, heads, True) + x
    return O.feed_forward(sd, p + ".ff", O._ln(sd, p + ".norm3", x)) + x


def spatial_transformer(sd, p, x, context, heads, depth=1):
    """oracle.spatial_transformer under the product's kv_pool_plan: where it answers None, the oracle's function itself."""
    n, c, h, w = x.shape
    w_in, w_out = sd[p + ".proj_in.weight"], sd[p + ".proj_out.weight"]
    if A.kv_pool_plan(h, w, w_in.shape[0]) is None:
        return _ORACLE_ST(sd, p, x, context, heads, depth)
    t = O._gn(sd, p + ".norm", x, 1e-6).permute(0, 2, 3, 1).reshape(n, h * w, c)
    t = F.linear(t, w_in.reshape(w_in.shape[0], -1), sd[p + ".proj_in.bias"])
    for i in range(depth):
        t = transformer_block(sd, f"{p}.transformer_blocks.{i}", t, context, heads, h, w, A.SATTN_KV_POOL)
    t = F.linear(t, w_out.reshape(w_out.shape[0], -1), sd[p + ".proj_out.bias"])
    return t.view(n, h, w, c).permute(0, 3, 1, 2) + x


_ORACLE_ST = O.spatial_transformer


@contextlib.contextmanager
def _pooled_transformers():
    """oracle.unet_forward reaches its spatial transformers through the module attribute: for the length of one call it is the function above"""
    O.spatial_transformer = spatial_transformer
    try:
        yield
    finally:
        O.spatial_transformer = _ORACLE_ST


def unet_forward(sd, hp, x, timesteps, context, fs=None, taps=None):
    """oracle.unet_forward with the pooled self-attention in every spatial transformer that kv_pool_plan pools"""
    with _pooled_transformers():
        return O.unet_forward(sd, hp, x, timesteps, context, fs, taps=taps)

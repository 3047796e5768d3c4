"""TEST INFRASTRUCTURE ONLY - the CPU stand-in for ops.layer_norm_pool2x2 (include/vcx.h vcx_layernorm_pool2x2_f16), written from its contract
on top of the existing stand-ins: the fp16 rows of tests/cpu_kernels.layer_norm, then the 2x2 mean in fp32 with one rounding
(tests/cpu_kernels.avgpool2x2) or the rows (2y, 2x).  tests/cpu_kernels.py is left as it is; the tests that need this install it."""
from tests import cpu_kernels as CK

POOL_MEAN, POOL_NEAREST = 0, 1


def layer_norm_pool2x2(x, gamma, beta, eps, n, H, W, mode):
    rows, C = x.shape
    assert rows == n * H * W and H % 2 == 0 and W % 2 == 0 and mode in (POOL_MEAN, POOL_NEAREST)
    a = CK.layer_norm(x, gamma, beta, eps).view(n, H, W, C)
    p = CK.avgpool2x2(a) if mode == POOL_MEAN else a[:, ::2, ::2]
    return p.reshape(n * (H // 2) * (W // 2), C).contiguous()


def install(monkeypatch):
    """tests/cpu_kernels.install plus the stand-in above."""
    from viewcrafter_amd import ops
    CK.install(monkeypatch)
    monkeypatch.setattr(ops, "layer_norm_pool2x2", layer_norm_pool2x2)

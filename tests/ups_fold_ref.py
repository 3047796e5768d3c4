"""References for the folded upsample convolution (tests/test_ups_fold.py, tests/test_ups_fold_gpu.py): nearest-2x + 3x3 / padding 1 as
four 2x2 convolutions on the source grid (viewcrafter_amd/packing.py pack_conv_ups_folded), evaluated in fp64 on channels-last tensors."""
import torch
import torch.nn.functional as F

# the three Upsample layers of the default workload (576x1024x25, CFG as one B = 2 forward): n, H, W, cin, cout
BENCH_LAYERS = {"36x64": (50, 36, 64, 640, 640), "18x32": (50, 18, 32, 1280, 1280), "9x16": (50, 9, 16, 1280, 1280)}


def nine_tap_ref(x, w, bias=None):
    """F.conv2d(F.interpolate(x, 2, 'nearest'), w, padding=1) in fp64: x [n, H, W, cin], w [cout, cin, 3, 3] -> [n, 2H, 2W, cout]."""
    up = F.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
    return F.conv2d(up, w.double(), None if bias is None else bias.double(), padding=1).permute(0, 2, 3, 1).contiguous()


def fold_classes(w):
    """[cout, cin, 3, 3] -> fp64 [2, 2, cout, cin, 2, 2]: the 2x2 kernel of parity class (a, b), written out tap by tap (not the einsum of
    the packing function): rows (w0, w1 + w2) for a = 0 and (w0 + w1, w2) for a = 1, columns alike."""
    w = w.double()
    rows = [torch.stack([w[:, :, 0], w[:, :, 1] + w[:, :, 2]], dim=2), torch.stack([w[:, :, 0] + w[:, :, 1], w[:, :, 2]], dim=2)]      # [cout, cin, 2, 3]
    out = torch.empty((2, 2) + tuple(w.shape[:2]) + (2, 2), dtype=torch.float64)
    for a in (0, 1):
        r = rows[a]
        out[a, 0] = torch.stack([r[..., 0], r[..., 1] + r[..., 2]], dim=3)
        out[a, 1] = torch.stack([r[..., 0] + r[..., 1], r[..., 2]], dim=3)
    return out


def folded_ref(x, w4, bias=None):
    """The four-class form in fp64: x [n, H, W, cin], w4 [2, 2, cout, cin, 2, 2] (any dtype) -> [n, 2H, 2W, cout]; class (a, b) reads source
    rows (i - 1 + a, i + a) and columns (j - 1 + b, j + b), zero outside, and writes output pixel (2i + a, 2j + b)."""
    n, H, W, _ = x.shape
    xp = F.pad(x.double().permute(0, 3, 1, 2), (1, 1, 1, 1))
    out = torch.empty((n, 2 * H, 2 * W, w4.shape[2]), dtype=torch.float64, device=x.device)
    for a in (0, 1):
        for b in (0, 1):
            y = F.conv2d(xp[:, :, a:a + H + 1, b:b + W + 1], w4[a, b].double().to(x.device), None if bias is None else bias.double())
            out[:, a::2, b::2] = y.permute(0, 2, 3, 1)
    return out


def unpack_folded(wf, cin):
    """[4, cout, 4 cin] as packed (slab-major where packing.conv_slab_major says so) -> [2, 2, cout, cin, 2, 2]."""
    from viewcrafter_amd.packing import conv_slab_major
    cout = wf.shape[1]
    if conv_slab_major(cin, 4):
        w = wf.view(4, cout, cin // 64, 4, 64).permute(0, 1, 2, 4, 3).reshape(4, cout, cin, 2, 2)
    else:
        w = wf.view(4, cout, 4, cin).permute(0, 1, 3, 2).reshape(4, cout, cin, 2, 2)
    return w.reshape(2, 2, cout, cin, 2, 2)

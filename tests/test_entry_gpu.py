"""The driver function and the command line on the MI355X.

  * `image_guided_synthesis` (reference utils/diffusion_utils.py:117-201) against a fixture written by the reference's
    own function (tests/golden/gen_golden.py::gen_igs): cond / uncond assembly from the CLIP towers and the Resampler,
    get_latent_z, CFG 7.5 with hybrid conditioning, two n_samples variants, decode - and the multi-condition variant;
  * `python inference.py --renderings ...` end to end as a subprocess: YAML -> instantiate_from_config -> strict checkpoint
    load -> setup_diffusion -> run_diffusion -> save_video (BASELINE configs[0] with the GPU in the loop).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.weights import NamedRandn, synth_input
from tests.util import SCHEDULE_BUFFERS, golden, load_synth, psnr, rel_l2, write_tiny_entry_files

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    sd = load_synth(m, skip=SCHEDULE_BUFFERS)
    g = golden("igs_tiny")
    have = sorted(k for k in m.state_dict().keys())
    assert have == [str(k) for k in g["igs_model_keys"]], "state-dict names differ from the reference's hybrid model"
    return m.to(DEV)


@pytest.mark.parametrize("tag,kw", [("cfg", dict(n_samples=2, multiple_cond_cfg=False, cfg_img=None)),
                                    ("multicond", dict(n_samples=1, multiple_cond_cfg=True, cfg_img=3.0))])
def test_image_guided_synthesis_vs_reference_golden(igs_model, tag, kw, monkeypatch):
    from tests.tiny_config import IGS_H, IGS_T, IGS_W
    from viewcrafter_amd.utils.diffusion_utils import image_guided_synthesis
    g = golden("igs_tiny")
    videos = torch.tanh(synth_input("igs_videos", (1, 3, IGS_T, IGS_H, IGS_W))).to(DEV)
    noise_shape = [1, 4, IGS_T, IGS_H // 8, IGS_W // 8]
    fake = NamedRandn(f"igs_{tag}_randn")
    monkeypatch.setattr(torch, "randn", fake)
    with torch.no_grad():
        vid = image_guided_synthesis(igs_model, [""], videos, noise_shape, ddim_steps=5, ddim_eta=1.0,
                                     unconditional_guidance_scale=7.5, fs=10, text_input=False,
                                     timestep_spacing="uniform_trailing", guidance_rescale=0.7, condition_index=[0], **kw)
    monkeypatch.undo()
    assert fake.calls == int(g[f"igs_{tag}_randn_calls"]), "Gaussian draws differ from the reference (count or order)"
    assert tuple(vid.shape) == (1, kw["n_samples"], 3, IGS_T, IGS_H, IGS_W) and vid.dtype == torch.float32
    ref = g[f"igs_{tag}_sub4"]
    sub = vid[..., ::4, ::4]
    e, p = rel_l2(sub, ref), psnr(sub, ref)
    print(f"image_guided_synthesis[{tag}]: decoded video rel-L2 vs the reference's own run = {e:.3e}, PSNR {p:.1f} dB")
    assert e <= 1.5e-2 and p >= 46.5      # measured 7.4e-3 / 52.7 dB (cfg), 4.1e-3 / 57.9 dB (multicond): ~2x the larger
    if kw["n_samples"] == 2:
        assert not torch.equal(vid[:, 0], vid[:, 1])          # two variants, two noise streams


def test_two_clips_per_gpu_on_two_streams_equal_the_plain_loop(igs_model):
    """viewcrafter_amd/interleave.py through parallel.run_sharded: three clips, two in flight at a time on their own HIP streams with the
    baton handed on after every DDIM step (eta = 1: a Gaussian draw per step and clip), against the same clips one after the other -
    bit-identical videos, the same generator state afterwards."""
    from tests.tiny_config import IGS_H, IGS_T, IGS_W
    from viewcrafter_amd import parallel
    from viewcrafter_amd.utils.diffusion_utils import image_guided_synthesis
    noise_shape = [1, 4, IGS_T, IGS_H // 8, IGS_W // 8]
    clips = [torch.tanh(synth_input(f"lanes_videos{i}", (1, 3, IGS_T, IGS_H, IGS_W))).to(DEV) for i in range(3)]

    def one(videos, index):
        torch.manual_seed(1234 + index)
        with torch.no_grad():
            return image_guided_synthesis(igs_model, [""], videos, noise_shape, ddim_steps=4, ddim_eta=1.0, unconditional_guidance_scale=7.5,
                                          fs=10, text_input=False, timestep_spacing="uniform_trailing", guidance_rescale=0.7,
                                          condition_index=[0])
    got = {}
    for lanes in (1, 2):
        torch.manual_seed(5)
        got[lanes] = parallel.run_sharded(one, clips, gather=False, lanes=lanes)
        torch.cuda.synchronize()
        got[lanes] = ([got[lanes][i].clone() for i in range(3)], torch.cuda.get_rng_state().clone(), torch.random.get_rng_state().clone())
    for a, b in zip(got[1][0], got[2][0]):
        assert torch.equal(a, b)
    assert torch.equal(got[1][1], got[2][1]) and torch.equal(got[1][2], got[2][2])
    assert not torch.equal(got[1][0][0], got[1][0][1])
    # ... and on a COLD model: every kernel-layout pack dropped, two lanes as the first call - the packs are then built on the
    # caller's stream before the lanes start (interleave.prepack) and the lanes wait on a hand-over event; a lane reading a pack that another
    # stream is still writing would show up here as differing bits
    for m in igs_model.modules():
        if hasattr(m, "_drop_packed"):
            m._drop_packed()
    torch.manual_seed(5)
    cold = parallel.run_sharded(one, clips, gather=False, lanes=2, model=igs_model)
    torch.cuda.synchronize()
    for i in range(3):
        assert torch.equal(got[1][0][i], cold[i]), "two lanes on a cold model differ from the plain loop"


def test_inference_cli_end_to_end(tmp_path):
    from viewcrafter_amd.utils.video_io import read_avi
    ypath, cpath, rpath, (T, H, W) = write_tiny_entry_files(tmp_path)
    out_dir = str(tmp_path / "out")
    cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "--renderings", rpath, "--config", ypath, "--ckpt_path", cpath,
           "--out_dir", out_dir, "--exp_name", "e", "--device", "cuda:0", "--ddim_steps", "5", "--video_length", str(T),
           "--height", str(H), "--width", str(W), "--prompt", "", "--seed", "123"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert ">>> model checkpoint loaded." in r.stdout
    res = torch.load(os.path.join(out_dir, "e", "diffusion0.pt"))
    assert tuple(res.shape) == (T, H, W, 3) and torch.isfinite(res).all()
    assert float(res.min()) >= -1.0 and float(res.max()) <= 1.0 and float(res.std()) > 1e-3       # viewcrafter.py:106 clamp
    vids = [f for f in os.listdir(os.path.join(out_dir, "e")) if f.startswith("diffusion0.") and f != "diffusion0.pt"]
    assert len(vids) == 1
    if vids[0].endswith(".avi"):
        frames, fps = read_avi(os.path.join(out_dir, "e", vids[0]))
        assert frames.shape == (T, H, W, 3) and fps == 8          # the reference writer's rate, pvd_utils.py:48
        expect = ((res + 1.0) / 2.0).clamp(0, 1).mul(255).round().to(torch.uint8).numpy()
        assert np.array_equal(frames, expect)
    # same seed, same command: the run is reproducible bit for bit (fixed summation orders everywhere)
    r2 = subprocess.run(cmd[:cmd.index("e")] + ["e2"] + cmd[cmd.index("e") + 1:], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r2.returncode == 0, r2.stderr[-4000:]
    assert torch.equal(torch.load(os.path.join(out_dir, "e2", "diffusion0.pt")), res)


def test_build_then_smoke_in_one_process():
    """`__graft_entry__.build()` binds libvcx.so before anything else has imported torch.  PyTorch-ROCm bundles its own HIP / HSA
    runtime under the same sonames, so `_lib.lib()` must make torch's copy the one in the process (it imports torch first):
    loaded the other way round every launch fails with "no ROCm-capable device is detected"."""
    code = ("import sys; import __graft_entry__ as g; g.build(); assert 'torch' in sys.modules; g.smoke(); "
            "from viewcrafter_amd import _lib; import ctypes; b = ctypes.create_string_buffer(64); "
            "assert _lib.lib().vcx_device_arch(b, 64) == 0 and b.value.startswith(b'gfx950'), b.value; print('ARCH', b.value.decode())")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "smoke OK" in r.stdout and "ARCH gfx950" in r.stdout


def test_rccl_collectives_of_the_sharded_launch_on_one_gpu(tmp_path):
    """The torchrun launch's control plane on the RCCL backend (`init_process_group("nccl", device_id=...)`, bucketed weight
    broadcast of GPU tensors, max-over-ranks timing all_reduce, checksum all_gather, clip gather, barrier) in a ONE-rank group on
    this box's GPU: the 2-rank tests run on gloo / CPU tensors, and no multi-GPU box is available to the test-suite."""
    code = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.getcwd())
from tests.tiny_config import TINY_UNET
from tests.util import load_synth
from viewcrafter_amd import parallel
from viewcrafter_amd.lvdm.modules.networks.openaimodel3d import UNetModel
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
rank, world = parallel.init_distributed()          # WORLD_SIZE=1 -> no group: build the one-rank RCCL group by hand, as bench.py does
assert (rank, world) == (0, 1)
dist.init_process_group("nccl", device_id=dev)
m = UNetModel(**TINY_UNET).eval(); load_synth(m); m = m.to(dev)
m.register_buffer("host_side_table", torch.arange(8, dtype=torch.float32))          # a buffer left on the host is staged
m._buffers["host_side_table"] = m._buffers["host_side_table"].cpu()
before = [p.detach().clone() for p in m.parameters()]
x = torch.randn(1, 8, 4, 16, 32, device=dev); ctx = torch.randn(1, 77 + 64, TINY_UNET["context_dim"], device=dev)
t, fs = torch.tensor([500], device=dev), torch.tensor([10], device=dev)
with torch.no_grad():
    y0 = m(x, t, context=ctx, fs=fs)               # packs fp16 copies, which the broadcast must invalidate
parallel.broadcast_module_(m, src=0, bucket_bytes=1 << 16, _force=True)          # small buckets: several broadcasts per dtype
assert all(torch.equal(a, b) for a, b in zip(before, m.parameters()))
assert torch.equal(m.host_side_table, torch.arange(8, dtype=torch.float32)) and m.host_side_table.device.type == "cpu"
with torch.no_grad():
    assert torch.equal(m(x, t, context=ctx, fs=fs), y0)
tmax = torch.tensor([1.25], dtype=torch.float64, device=dev); dist.all_reduce(tmax, op=dist.ReduceOp.MAX); assert float(tmax) == 1.25
chk = torch.stack([p.detach().double().sum() for p in m.parameters()]).sum().reshape(1)
allc = [torch.empty_like(chk)]; dist.all_gather(allc, chk); assert torch.equal(allc[0], chk)
clip = (torch.rand(3, 16, 24, 3, device=dev) * 255).to(torch.uint8)
got = parallel.gather_results({0: clip}, 1, _force=True)
assert len(got) == 1 and torch.equal(got[0], clip)
torch.cuda.synchronize(); dist.barrier()
parallel.shutdown()
print("RCCL-ONE-RANK-OK")
"""
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29533",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "RCCL-ONE-RANK-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_bench_gpus_2_launch_line_on_this_one_gpu_is_a_marked_smoke_test():
    """The driver's multi-GPU command, `python bench.py --gpus 2`, executed for real on this box's ONE GPU with VCX_BENCH_SHARE_GPU=1:
    bench.py re-executes itself under `python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1`, both ranks build
    the full-width 320x512 model on the shared device, run the barrier-bracketed timed region, decode and gather their clips - and
    the ONE line rank 0 prints says it is not a measurement (RCCL cannot place two ranks on one device, so the control plane is
    gloo here; the RCCL collectives themselves are covered by test_rccl_collectives_of_the_sharded_launch_on_one_gpu).  What no
    test can give on a one-GPU box is a scaling number: SCALE_rNN.json is the driver's to measure."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(VCX_BENCH_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--workload",
                        "ViewCrafter_25_512_320x512x25", "--full", "--no-cpu-baseline", "--no-gpu-legs", "--no-extra", "--no-video"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = lines[0]
    assert out["n_gpus"] == 2 and len(out["per_rank_steps_per_s"]) == 2 and out["scaling"] == "weak"
    assert "SMOKE TEST" in out["backend"] and "not a measurement" in out["backend"]
    assert out["value"] > 0 and out["gather_s"] is not None
    assert "torch.distributed.run" in r.stderr


def test_plain_bench_run_prints_the_headline_only_and_dumps_the_last_step(tmp_path):
    """`python bench.py` without --full: warm-up, timed steps and the contract line - no roofline, telemetry or baselines - and
    --dump-outputs writes the last timed step's x_prev / pred_x0 as float32 .npy files of the latent's shape."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    dump = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--workload",
                        "ViewCrafter_25_512_320x512x25", "--dump-outputs", str(dump)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"):
        assert k in out, k
    assert out["steps"] == 2 and out["warmup"] == 1 and out["n_gpus"] == 1 and out["full"] is False
    assert out["unit"] == "DDIM steps/s" and out["higher_is_better"] is True and out["dtype"] == "f16"
    assert out["value"] == pytest.approx(1e3 / out["ms_per_step"], rel=1e-6)
    for k in ("roofline", "telemetry", "cpu_baseline", "gpu_eager_baseline", "parity", "extra", "sec_per_video"):
        assert k not in out, k
    assert sorted(os.listdir(dump)) == ["pred_x0.npy", "x_prev.npy"]
    for name in ("x_prev", "pred_x0"):
        a = np.load(dump / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == (1, 4, 25, 40, 64) and np.isfinite(a).all(), name

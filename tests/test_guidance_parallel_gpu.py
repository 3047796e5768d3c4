"""One video on several GPUs (VCX_GUIDANCE_PARALLEL) on the MI355X.

  * the sampler's split route - one B = b forward of ONE conditioning per rank and step, the outputs exchanged - against the default
    route (the stacked forward with the shared CFG prefix) in one process, with a stand-in group that evaluates the other positions
    locally: bit-identical x_prev / pred_x0 at every step, CFG and multi-condition guidance, b = 1 and b = 2;
  * the real command line: 2 (CFG) and 3 (multi-condition) ranks of `python -m torch.distributed.run ... inference.py` on this box's
    ONE GPU (VCX_SHARE_GPU=1 test mode, gloo control plane) write the video of the one-process command, also with VCX_CLIP_BATCH=2;
  * GuidanceGroup.exchange on a one-rank RCCL group: the all_gather_into_tensor path the gloo launches do not take."""
import os
import subprocess
import sys

import pytest
import torch

from oracle.weights import synth_input
from tests.tiny_config import TINY_UNET, tiny_model_params
from tests.util import SCHEDULE_BUFFERS, load_synth, write_tiny_entry_files

pytestmark = pytest.mark.gpu
# Processes on the GPU: a launch of this file adds at most three (its ranks) to the pytest process, which holds the device anyway once
# any GPU test module of the suite has run; the launches are never concurrent.
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 5


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _assert_every_rank_ran_its_own_forward(stdout, ranks, batch):
    """The line every working rank prints at the end (GuidanceGroup.report; counted in the sampler's split route and in exchange): one
    forward per step, of `batch` videos, under the conditioning of the rank's position, one exchange each - a launch whose sampler never
    received the group would report nothing (or zeros) while still writing the right video."""
    for r in range(ranks):
        want = (f"[guidance-parallel] rank {r} group 0 position {r}: {STEPS} steps, {STEPS} forwards of batch {batch} under its own "
                f"conditioning, {STEPS} exchanges")
        assert stdout.count(want) == 1, f"rank {r}: no line {want!r} in\n" + "\n".join(
            ln for ln in stdout.splitlines() if "[guidance-parallel]" in ln)
LAUNCH_ENV = ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "VCX_GUIDANCE_PARALLEL", "VCX_DIST_BACKEND",
              "VCX_SHARE_GPU", "VCX_CLIP_BATCH", "VCX_CLIPS_PER_GPU")


@pytest.fixture(scope="module")
def model():
    from viewcrafter_amd.config import Config
    from viewcrafter_amd.utils.diffusion_utils import instantiate_from_config
    params = Config.wrap(tiny_model_params("lvdm.modules.networks.openaimodel3d.UNetModel", "lvdm.models.autoencoder.AutoencoderKL"))
    m = instantiate_from_config(Config(target="lvdm.models.ddpm3d.VIPLatentDiffusion", params=params)).eval()
    load_synth(m, skip=SCHEDULE_BUFFERS)
    return m.to(DEV)


# ------------------------------------------------------------------------------------------------------ 1. split route vs default route
class _StandInGroup:
    """A test helper, not product code: `exchange` evaluates the conditionings of the OTHER positions here, one after the other, on
    the step's own inputs (recorded by the apply_model spy below)."""

    def __init__(self, model, conds, position):
        self.size, self.position, self.index = len(conds), position, 0
        self.conds, self.real, self.last, self.own_calls = conds, model.apply_model, None, []

    def spy(self, x, t, c, **kw):
        self.own_calls.append((x.shape[0], "cfg_repeat" in kw, c is self.conds[self.position]))
        self.last = (x, t, kw)
        return self.real(x, t, c, **kw)

    def exchange(self, v):
        x, t, kw = self.last
        return [v if i == self.position else self.real(x, t, self.conds[i], **kw) for i in range(self.size)]

    @staticmethod
    def checksum(x):
        return None

    def check_equal(self, x, **kw):
        pass


def _trajectory(model, multicond, b, position=None):
    """x_prev and pred_x0 of all 5 steps (eta 1, rescale 0.7): default route (position None) or the split route of one position."""
    from viewcrafter_amd.utils.diffusion_utils import _sampler
    t, h, w, cd = 4, 32, 16, TINY_UNET["context_dim"]
    cat = synth_input("gp_cat", (b, 4, t, h, w), scale=0.8).to(DEV)
    ctx, uctx = synth_input("gp_ctx", (b, 77 + 16 * t, cd)).to(DEV), synth_input("gp_uctx", (b, 77 + 16 * t, cd)).to(DEV)
    cond = {"c_crossattn": [ctx], "c_concat": [cat]}
    uc = {"c_crossattn": [uctx], "c_concat": [cat]}
    uc2 = {"c_crossattn": [torch.cat([uctx[:, :77], ctx[:, 77:]], 1)], "c_concat": [cat]} if multicond else None
    sampler = _sampler(model, multicond)
    group = None
    if position is not None:
        group = _StandInGroup(model, [cond, uc, uc2][:3 if multicond else 2], position)
        sampler.guidance_group = group
        model.apply_model = group.spy
    calls = []
    if group is None:
        real = model.apply_model

        def count(x, ts, c, **kw):
            calls.append((x.shape[0], "cfg_repeat" in kw))
            return real(x, ts, c, **kw)
        model.apply_model = count
    torch.manual_seed(4321)
    try:
        with torch.no_grad():
            _, inter = sampler.sample(S=STEPS, conditioning=cond, batch_size=b, shape=[4, t, h, w], verbose=False,
                                      unconditional_guidance_scale=7.5, unconditional_conditioning=uc, eta=1.0,
                                      cfg_img=3.0 if multicond else None, mask=None, x0=None, fs=torch.tensor([10] * b, device=DEV),
                                      timestep_spacing="uniform_trailing", guidance_rescale=0.7, log_every_t=1,
                                      unconditional_conditioning_img_nonetext=uc2)
    finally:
        del model.apply_model            # the instance attribute: the class's method is back
    torch.cuda.synchronize()
    return inter["x_inter"], inter["pred_x0"], (group.own_calls if group is not None else calls)


@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("multicond", [False, True])
def test_split_route_equals_the_batched_shared_prefix_route(model, multicond, b):
    want_x, want_p, calls = _trajectory(model, multicond, b)
    assert calls == [(b, True)] * STEPS, "the default route is the ONE stacked forward with the shared prefix"
    assert len(want_x) == STEPS + 1 and all(torch.isfinite(x).all() for x in want_x)
    assert not torch.equal(want_x[1], want_x[2])
    for position in range(3 if multicond else 2):
        got_x, got_p, own = _trajectory(model, multicond, b, position)
        assert own == [(b, False, True)] * STEPS, f"position {position}: {own}"
        for i in range(STEPS + 1):
            assert torch.equal(got_x[i], want_x[i]), f"position {position}: x_prev of step {i} differs in {int((got_x[i] != want_x[i]).sum())} elements"
            assert torch.equal(got_p[i], want_p[i]), f"position {position}: pred_x0 of step {i} differs"


# ------------------------------------------------------------------------------------------------------ 2. the command line
def _cli(tmp_path, tag, renders, ypath, cpath, thw, ranks=None, extra=(), env_extra=None):
    """`inference.py --renderings ...` as one process (ranks None) or under torch.distributed.run with the guidance-parallel test
    environment; returns (the diffusion<i>.pt tensors, stdout)."""
    T, H, W = thw
    env = {k: v for k, v in os.environ.items() if k not in LAUNCH_ENV}
    head = [sys.executable]
    if ranks is not None:
        head += ["-m", "torch.distributed.run", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1", "--master-port", str(_free_port())]
        env.update(VCX_GUIDANCE_PARALLEL="1", VCX_DIST_BACKEND="gloo", VCX_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.update(env_extra or {})
    out_dir = str(tmp_path / f"out_{tag}")
    cmd = head + [os.path.join(ROOT, "inference.py"), "--renderings", ",".join(renders), "--config", ypath, "--ckpt_path", cpath,
                  "--out_dir", out_dir, "--exp_name", "e", "--device", "cuda:0", "--ddim_steps", str(STEPS), "--video_length", str(T),
                  "--height", str(H), "--width", str(W), "--prompt", "", "--seed", "123"] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return [torch.load(os.path.join(out_dir, "e", f"diffusion{i}.pt")) for i in range(len(renders))], r.stdout


@pytest.fixture(scope="module")
def entry(tmp_path_factory):
    from tests.tiny_config import IGS_H, IGS_T, IGS_W
    tmp = tmp_path_factory.mktemp("guidance_parallel")
    ypath, cpath, rpath, thw = write_tiny_entry_files(tmp)
    second = os.path.join(str(tmp), "renders1.pt")
    torch.save(torch.rand(IGS_T, IGS_H, IGS_W, 3, generator=torch.Generator().manual_seed(51)), second)
    return tmp, ypath, cpath, [rpath, second], thw


@pytest.fixture(scope="module")
def plain_two_clips(entry):
    """The one-process plain loop over both clips, once: clip 0 of it is the one-process run of the first clip alone."""
    tmp, ypath, cpath, renders, thw = entry
    return _cli(tmp, "plain", renders, ypath, cpath, thw)[0]


def test_two_ranks_write_the_one_process_video(entry, plain_two_clips):
    tmp, ypath, cpath, renders, thw = entry
    got, stdout = _cli(tmp, "split2", renders[:1], ypath, cpath, thw, ranks=2)
    assert stdout.count("[guidance-parallel] 1 groups of 2: [[0, 1]], idle []") == 1, stdout[-2000:]
    _assert_every_rank_ran_its_own_forward(stdout, 2, batch=1)
    assert torch.equal(got[0], plain_two_clips[0]), f"{int((got[0] != plain_two_clips[0]).sum())} elements differ"
    assert float(got[0].std()) > 1e-3


def test_three_ranks_write_the_one_process_video_with_multi_condition_guidance(entry):
    tmp, ypath, cpath, renders, thw = entry
    extra = ["--multiple_cond_cfg", "--cfg_img", "3.0"]
    want, plain_out = _cli(tmp, "plain_mc", renders[:1], ypath, cpath, thw, extra=extra)
    got, stdout = _cli(tmp, "split3", renders[:1], ypath, cpath, thw, ranks=3, extra=extra)
    assert "[guidance-parallel]" not in plain_out
    assert stdout.count("[guidance-parallel] 1 groups of 3: [[0, 1, 2]], idle []") == 1, stdout[-2000:]
    _assert_every_rank_ran_its_own_forward(stdout, 3, batch=1)
    assert torch.equal(got[0], want[0]), f"{int((got[0] != want[0]).sum())} elements differ"


def test_two_ranks_two_clips_batched_write_the_plain_loops_videos(entry, plain_two_clips):
    tmp, ypath, cpath, renders, thw = entry
    got, stdout = _cli(tmp, "split2_batch", renders, ypath, cpath, thw, ranks=2, env_extra={"VCX_CLIP_BATCH": "2"})
    assert stdout.count("[guidance-parallel] 1 groups of 2") == 1
    _assert_every_rank_ran_its_own_forward(stdout, 2, batch=2)          # both clips in ONE forward of the rank's conditioning
    for i in range(2):
        assert torch.equal(got[i], plain_two_clips[i]), f"diffusion{i}.pt differs from the plain loop's"
    assert not torch.equal(got[0], got[1])


# ------------------------------------------------------------------------------------------------------ 3. RCCL, one rank
def test_exchange_on_a_one_rank_rccl_group(tmp_path):
    code = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.getcwd())
from viewcrafter_amd import parallel
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
assert parallel.init_distributed() == (0, 1)        # WORLD_SIZE=1 -> no group: the one-rank RCCL group is built by hand
dist.init_process_group("nccl", device_id=dev)
group = parallel.GuidanceGroup(1, 0, 0, dist.new_group([0]))
v1 = torch.randn(1, 4, 4, 32, 16, device=dev); v2 = torch.randn(1, 4, 4, 32, 16, device=dev)
warm = group.exchange(v1)                            # communicator and buffer are created here
torch.cuda.synchronize()
torch.cuda.set_sync_debug_mode("error")              # any host synchronisation raises from here on
out1 = group.exchange(v1); ptr1 = out1[0].data_ptr(); keep1 = out1[0].clone()
out2 = group.exchange(v2); ptr2 = out2[0].data_ptr()
torch.cuda.set_sync_debug_mode("default")
torch.cuda.synchronize()
assert len(out1) == 1 and len(out2) == 1 and out1[0].shape == v1.shape
assert torch.equal(keep1, v1) and torch.equal(out2[0], v2)
assert ptr1 == ptr2 == warm[0].data_ptr() and ptr1 != v1.data_ptr(), "one buffer, reused across the calls"
group.check_equal(v2)                                # the end-of-loop checksum on RCCL: one all_gather, one host sync
parallel.shutdown()
print("RCCL-EXCHANGE-OK")
"""
    env = {k: v for k, v in os.environ.items() if k not in LAUNCH_ENV}
    env.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RCCL-EXCHANGE-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]

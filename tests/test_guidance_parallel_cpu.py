"""One video on several GPUs (VCX_GUIDANCE_PARALLEL, viewcrafter_amd/parallel.py), the host side on gloo ranks: the rank layout, the
switch and what it refuses, the sampler's split route on the tiny model (launchers of tests/cpu_kernels.py, as tests/test_hostgraph_cpu.py
installs them) - one forward of the rank's own conditioning per step, the final latent bit-equal to the one-process run's - the
end-of-loop checksum, and `inference.main` with the stub diffusion model of tests/test_entry_cpu.py."""
import os
import sys
import types

import pytest
import torch
import torch.multiprocessing as mp

from tests.test_entry_cpu import _free_port, _StubModel
from viewcrafter_amd import clip_batch, parallel

SEED = 77
STEPS = 4
# b, C, T, h, w.  16 rows per video at the deepest UNet level: tests/cpu_kernels.py::gemm is one `X @ W.t()` over all M rows of a call, and
# the host's single-threaded sgemm rounds a row differently at M = 12 than at M = 4 (measured: 4 rows, K = 256, three stacked copies
# against one: up to 3e-5; two copies: equal; 16, 64, 256 rows: equal at 2 and 3 copies).  At a 16 x 8 latent (4 rows per video at the
# deepest level) the one-process stacked forward of THREE videos therefore leaves the bits of a B = 1 forward (final latents 1.1e-1
# apart after 4 steps, all three ranks still equal to each other) - a property of the stand-ins, not of the product's kernels
# (tests/test_batch_invariance_gpu.py).  At 32 x 16 every route gives the same bits on the stand-ins as well.
LATENT = (1, 4, 2, 32, 16)
TIMEOUT = 300
# The stand-in launchers are plain PyTorch: the host BLAS picks its summation order by thread count (and, with many threads, by the
# batch), which the product's kernels do not (tests/test_batch_invariance_gpu.py).  The one-process run and every rank therefore use
# the same, single-threaded BLAS.
THREADS = 1


# ------------------------------------------------------------------------------------------------------ 1. layout
def test_guidance_layout():
    assert parallel.guidance_layout(2, 2) == (1, [0, 0], [0, 1], [])
    n, group_of, pos_of, idle = parallel.guidance_layout(8, 2)
    assert n == 4 and group_of == [0, 0, 1, 1, 2, 2, 3, 3] and pos_of == [0, 1] * 4 and idle == []
    n, group_of, pos_of, idle = parallel.guidance_layout(8, 3)
    assert n == 2 and idle == [6, 7]
    assert [[r for r in range(8) if group_of[r] == g] for g in range(n)] == [[0, 1, 2], [3, 4, 5]]
    assert pos_of == [0, 1, 2, 0, 1, 2, None, None] and group_of[6:] == [None, None]
    with pytest.raises(ValueError, match="needs at least 2 ranks"):
        parallel.guidance_layout(1, 2)
    with pytest.raises(ValueError, match="nothing to split"):
        parallel.guidance_layout(4, 1)
    with pytest.raises(ValueError, match="nothing to split"):
        parallel.guidance_layout(4, clip_batch.guidance_copies(1.0))
    assert parallel.describe_layout(2, 2) == "[guidance-parallel] 1 groups of 2: [[0, 1]], idle []"
    assert parallel.describe_layout(8, 3) == "[guidance-parallel] 2 groups of 3: [[0, 1, 2], [3, 4, 5]], idle [6, 7]"


def test_clips_are_owned_by_groups_without_a_launch():
    """run_sharded with a group: group g of G runs clips g, g + G, ...; an idle rank (index None) runs nothing."""
    for index, want in ((0, [0, 2, 4]), (1, [1, 3]), (None, [])):
        seen = []
        g = parallel.GuidanceGroup(2, 0 if index is not None else None, index, None, n_groups=2)
        parallel.run_sharded(lambda item, i: seen.append(i), list("abcde"), gather=False, group=g)
        assert seen == want
        seen = []
        parallel.run_sharded_batched(lambda items, idx: [seen.append(list(idx))] * len(idx), list("abcde"), 2, gather=False, group=g)
        assert seen == ([want[:2], want[2:]] if len(want) > 2 else ([want] if want else []))


def _spawn(target, world, args):
    """`world` processes of target(rank, world, port, *args); every one must exit 0 within TIMEOUT (a straggler is killed)."""
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port) + tuple(args)) for r in range(world)]
    for p in procs:
        p.start()
    codes = []
    for p in procs:
        p.join(timeout=TIMEOUT)
        if p.is_alive():
            p.kill()
            p.join()
            codes.append("hung")
        else:
            codes.append(p.exitcode)
    assert codes == [0] * world, codes


def _rank_env(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(THREADS)


def _gather_worker(rank, world, port, tmp):
    _rank_env(rank, world, port)
    parallel.init_distributed(backend="gloo")
    group = parallel.build_guidance_group(2)
    ran = []

    def fn(item, index):
        ran.append(index)
        return torch.tensor([float(item), float(index)])
    out = parallel.run_sharded(fn, [10, 11, 12, 13, 14], gather=True, group=group)
    torch.save(dict(ran=ran, out=out, index=group.index, position=group.position, ranks=group.ranks), os.path.join(tmp, f"g{rank}.pt"))
    parallel.shutdown()


def test_leaders_gather_returns_the_clips_in_clip_order(tmp_path):
    """5 ranks, CFG: groups [0, 1] and [2, 3], rank 4 idle.  Both ranks of a group run the group's clips; the gather runs over the
    leaders (ranks 0 and 2) only and rank 0 holds the results in clip order."""
    _spawn(_gather_worker, 5, (str(tmp_path),))
    got = [torch.load(tmp_path / f"g{r}.pt") for r in range(5)]
    assert [g["ran"] for g in got] == [[0, 2, 4], [0, 2, 4], [1, 3], [1, 3], []]
    assert [(g["index"], g["position"]) for g in got] == [(0, 0), (0, 1), (1, 0), (1, 1), (None, None)]
    assert got[0]["ranks"] == [0, 1] and got[3]["ranks"] == [2, 3]
    assert all(g["out"] is None for g in got[1:])
    assert torch.equal(torch.stack(got[0]["out"]), torch.tensor([[10., 0.], [11., 1.], [12., 2.], [13., 3.], [14., 4.]]))


# ------------------------------------------------------------------------------------------------------ 2. the switch
def test_switch_parsing_and_refusals():
    assert parallel.guidance_parallel_from_env({}) is False
    assert parallel.guidance_parallel_from_env({"VCX_GUIDANCE_PARALLEL": "0"}) is False
    assert parallel.guidance_parallel_from_env({"VCX_GUIDANCE_PARALLEL": ""}) is False
    assert parallel.guidance_parallel_from_env({"VCX_GUIDANCE_PARALLEL": "1"}) is True
    assert parallel.guidance_parallel_from_env({"VCX_GUIDANCE_PARALLEL": "1", "VCX_CLIP_BATCH": "4"}) is True
    assert parallel.guidance_parallel_from_env({"VCX_GUIDANCE_PARALLEL": "0", "VCX_CLIPS_PER_GPU": "2"}) is False
    with pytest.raises(ValueError, match="VCX_GUIDANCE_PARALLEL=1 and VCX_CLIPS_PER_GPU=2 cannot be combined"):
        parallel.guidance_parallel_from_env({"VCX_GUIDANCE_PARALLEL": "1", "VCX_CLIPS_PER_GPU": "2"})
    with pytest.raises(ValueError, match="must be 0 or 1"):
        parallel.guidance_parallel_from_env({"VCX_GUIDANCE_PARALLEL": "yes"})


def test_driver_refuses_two_streams_and_caps_the_clip_batch_with_one_copy(monkeypatch):
    import viewcrafter
    vc = viewcrafter.ViewCrafter.__new__(viewcrafter.ViewCrafter)
    opts = types.SimpleNamespace(seed=SEED, unconditional_guidance_scale=7.5, multiple_cond_cfg=False, cfg_img=None)
    unet = types.SimpleNamespace()
    model = types.SimpleNamespace(model=types.SimpleNamespace(diffusion_model=unet))
    vc.__dict__.update(opts=opts, _ref=None, diffusion=model, noise_shape=[1, 4, 25, 72, 128])
    monkeypatch.setenv("VCX_GUIDANCE_PARALLEL", "1")
    monkeypatch.setenv("VCX_CLIPS_PER_GPU", "2")
    with pytest.raises(ValueError, match="VCX_GUIDANCE_PARALLEL=1 and VCX_CLIPS_PER_GPU=2 cannot be combined"):
        vc.run_diffusion_many([torch.zeros(1)])
    monkeypatch.delenv("VCX_CLIPS_PER_GPU")
    monkeypatch.setenv("VCX_CLIP_BATCH", "4")
    group = parallel.GuidanceGroup(2, 0, 0, None)
    vc.__dict__["_guidance"] = group
    seen = {}

    def cap(unet_, noise_shape, copies):
        seen["copies"] = copies
        return 7

    def batched(fn, items, k, gather=True, group=None):
        seen.update(k=k, group=group, split_inside=vc.__dict__.get("_split"))
        return "ran"
    monkeypatch.setattr(clip_batch, "max_clips_per_forward", cap)
    monkeypatch.setattr(parallel, "run_sharded_batched", batched)
    assert vc.run_diffusion_many([torch.zeros(1)] * 5) == "ran"
    assert seen == dict(copies=1, k=4, group=group, split_inside=group)
    assert vc.__dict__["_split"] is None and vc._split_kw() == {}


# ------------------------------------------------------------------------------------------------------ 3. / 4. the sampler
def _tiny_model():
    from tests.tiny_config import tiny_model_params
    from tests.util import SCHEDULE_BUFFERS, load_synth
    from viewcrafter_amd.config import Config
    from viewcrafter_amd.utils.diffusion_utils import instantiate_from_config
    params = Config.wrap(tiny_model_params("lvdm.modules.networks.openaimodel3d.UNetModel", "lvdm.models.autoencoder.AutoencoderKL"))
    m = instantiate_from_config(Config(target="lvdm.models.ddpm3d.VIPLatentDiffusion", params=params)).eval()
    load_synth(m, skip=SCHEDULE_BUFFERS)
    return m


def _install_cpu_launchers(monkeypatch):
    from tests import cpu_kernels
    from tests.test_hostgraph_cpu import _ddim_step_cpu
    from viewcrafter_amd import ops
    cpu_kernels.install(monkeypatch)
    monkeypatch.setattr(ops, "ddim_step", _ddim_step_cpu)


def _sample(model, multicond, group, perturb=False):
    """4 steps, eta 1, rescale 0.7 after manual_seed(SEED).  Returns (final latent, [(batch, 'cfg_repeat' given, conditioning number)]
    of every apply_model call)."""
    from oracle.weights import synth_input
    from tests.tiny_config import TINY_UNET
    from viewcrafter_amd.utils.diffusion_utils import _sampler
    b, _, t, h, w = LATENT
    cd = TINY_UNET["context_dim"]
    cat = synth_input("gp_cat", (b, 4, t, h, w), scale=0.8)
    ctx, uctx = synth_input("gp_ctx", (b, 77 + 16 * t, cd)), synth_input("gp_uctx", (b, 77 + 16 * t, cd))
    cond = {"c_crossattn": [ctx], "c_concat": [cat]}
    uc = {"c_crossattn": [uctx], "c_concat": [cat]}
    uc2 = {"c_crossattn": [torch.cat([uctx[:, :77], ctx[:, 77:]], 1)], "c_concat": [cat]} if multicond else None
    conds = [cond, uc, uc2]
    calls = []
    real = model.apply_model

    def spy(x, ts, c, **kw):
        calls.append((x.shape[0], "cfg_repeat" in kw, next((i for i, k in enumerate(conds) if k is c), None)))
        return real(x, ts, c, **kw)
    model.apply_model = spy
    sampler = _sampler(model, multicond, group)
    torch.manual_seed(SEED)
    x_T = None
    if perturb:
        x_T = torch.randn(LATENT)
        x_T.view(-1)[5] = torch.nextafter(x_T.view(-1)[5], torch.tensor(float("inf")))
    try:
        with torch.no_grad():
            out, _ = sampler.sample(S=STEPS, conditioning=cond, batch_size=b, shape=list(LATENT[1:]), verbose=False,
                                    unconditional_guidance_scale=7.5, unconditional_conditioning=uc, eta=1.0,
                                    cfg_img=3.0 if multicond else None, mask=None, x0=None, fs=torch.tensor([10] * b),
                                    timestep_spacing="uniform", guidance_rescale=0.7, x_T=x_T,
                                    unconditional_conditioning_img_nonetext=uc2)        # "uniform": the first step is below t = 999,
    # where the zero-terminal-SNR schedule of the tiny model would erase x_T - and the one-ulp perturbation - from the trajectory
    finally:
        model.apply_model = real
    return out, calls


_REFERENCE = {}


def _reference(multicond):
    """The one-process run, once per guidance kind."""
    if multicond not in _REFERENCE:
        threads = torch.get_num_threads()
        torch.set_num_threads(THREADS)
        try:
            with pytest.MonkeyPatch.context() as mp_:
                _install_cpu_launchers(mp_)
                _REFERENCE[multicond] = _sample(_tiny_model(), multicond, None)
        finally:
            torch.set_num_threads(threads)
    return _REFERENCE[multicond]


def _sampler_worker(rank, world, port, tmp, multicond, perturb_rank):
    _rank_env(rank, world, port)
    _install_cpu_launchers(pytest.MonkeyPatch())
    parallel.init_distributed(backend="gloo")
    group = parallel.build_guidance_group(world)
    res = dict(position=group.position, error=None, out=None, calls=None)
    try:
        res["out"], res["calls"] = _sample(_tiny_model(), multicond, group, perturb=(rank == perturb_rank))
    except RuntimeError as e:
        res["error"] = str(e)
    res["report"] = group.report(rank)
    torch.save(res, os.path.join(tmp, f"s{rank}.pt"))
    parallel.shutdown()


@pytest.mark.parametrize("multicond", [False, True])
def test_each_rank_runs_one_forward_of_its_own_conditioning_and_the_latent_is_the_one_process_latent(tmp_path, multicond):
    """2 ranks with CFG, 3 with multi-condition guidance; the reference is the one-process run on its default route (one stacked
    forward with the shared prefix).

    The latent (LATENT) is the smallest at which the CPU stand-ins themselves are batch-invariant: see the note at LATENT."""
    world = 3 if multicond else 2
    want, want_calls = _reference(multicond)
    # the default route: one stacked forward per step (the shared prefix: batch b with cfg_repeat, a stacked conditioning)
    assert want_calls == [(LATENT[0], True, None)] * STEPS and torch.isfinite(want).all()
    _spawn(_sampler_worker, world, (str(tmp_path), multicond, -1))
    for r in range(world):
        got = torch.load(tmp_path / f"s{r}.pt")
        assert got["error"] is None, got["error"]
        assert got["position"] == r
        assert got["calls"] == [(LATENT[0], False, r)] * STEPS, f"rank {r}: {got['calls']}"
        assert got["report"] == (f"[guidance-parallel] rank {r} group 0 position {r}: {STEPS} steps, {STEPS} forwards of batch {LATENT[0]} "
                                 f"under its own conditioning, {STEPS} exchanges")        # the line the command-line tests read
        print(f"rank {r} of {world}: max |final latent - one-process run| = {float((got['out'] - want).abs().max()):.3e}")
        assert torch.equal(got["out"], want), f"rank {r}: the final latent differs from the one-process run's"


def test_non_dict_conditionings_split_the_same_way():
    """The route does not depend on `_batchable`: tensor conditionings go to conds[position] as well."""
    from viewcrafter_amd.lvdm.models.samplers.ddim import DDIMSampler

    class Group:
        size, position = 2, 1

        def exchange(self, v):
            return [v - 1.0, v]
    seen = []
    model = types.SimpleNamespace(num_timesteps=1000, apply_model=lambda x, t, c, **kw: (seen.append((c, dict(kw))), x + c)[1])
    s = DDIMSampler(model)
    assert s.guidance_group is None
    s.guidance_group = Group()
    c, uc = torch.tensor([1.0]), torch.tensor([2.0])
    assert not s._batchable(c, uc)
    v_c, v_u, v_i, cfg_img = s._model_outputs(torch.zeros(1), torch.zeros(1), c, uc, 7.5, {"fs": 3})
    assert len(seen) == 1 and seen[0][0] is uc and seen[0][1] == {"fs": 3}
    assert float(v_c) == 1.0 and float(v_u) == 2.0 and v_i is None
    s.guidance_group = types.SimpleNamespace(size=3, position=0)
    with pytest.raises(ValueError, match="3 ranks"):
        s._model_outputs(torch.zeros(1), torch.zeros(1), c, uc, 7.5, {})


def test_a_rank_that_starts_one_ulp_away_makes_the_checksum_raise_on_both_ranks(tmp_path):
    _spawn(_sampler_worker, 2, (str(tmp_path), False, 1))
    for r in range(2):
        got = torch.load(tmp_path / f"s{r}.pt")
        assert got["out"] is None and got["error"] is not None, f"rank {r} did not raise"
        assert "differs between the ranks" in got["error"] and "ranks [1] do not hold the bits of rank 0" in got["error"], got["error"]


# ------------------------------------------------------------------------------------------------------ 5. inference.main
def _stub_entry(rank, expect_group):
    """inference.main's collaborators replaced as in tests/test_entry_cpu.py: every rank starts with different "weights" (rank 0's
    arrive by broadcast), the synthesis stand-in depends on the clip, the weights and the noise it draws."""
    import viewcrafter

    def build(config, device="cpu", ckpt_path=None, **kw):
        assert (ckpt_path is not None) == (rank == 0), "only rank 0 reads the checkpoint"
        state = torch.random.get_rng_state()
        torch.manual_seed(1000 + rank)
        m = _StubModel()
        torch.random.set_rng_state(state)        # like the real constructor + checkpoint load: the same draws on every rank
        return m

    def synth(model, prompts, videos, noise_shape, *a, guidance_group=None, **kw):
        if expect_group:
            assert guidance_group is not None and guidance_group.size == 2 and guidance_group.position == rank
        else:
            assert guidance_group is None
        tag = 0.1 * videos.mean() + 0.01 * model.w.detach().sum() + 0.01 * torch.randn(())
        if guidance_group is not None:
            both = guidance_group.exchange(tag.reshape(1))
            guidance_group.check_equal(torch.stack(both))
            tag = both[1 - rank][0]                  # the OTHER rank's value: equal only if both drew the same noise
        return (videos * 0 + tag).unsqueeze(1)
    viewcrafter.build_diffusion_model = build
    viewcrafter.image_guided_synthesis = synth


def _argv(tmp, exp):
    return ["--config", "none.yaml", "--ckpt_path", os.path.join(tmp, "ckpt"), "--out_dir", os.path.join(tmp, "out"), "--exp_name", exp,
            "--device", "cpu", "--video_length", "3", "--height", "16", "--width", "16", "--seed", "11",
            "--renderings", os.path.join(tmp, "r0.pt")]


def _entry_worker(rank, world, port, tmp):
    _rank_env(rank, world, port)
    os.environ["VCX_GUIDANCE_PARALLEL"] = "1"
    sys.stdout = open(os.path.join(tmp, f"stdout{rank}.txt"), "w")
    import inference
    _stub_entry(rank, expect_group=True)
    out = inference.main(_argv(tmp, "split"))
    assert (out is None) == (rank != 0)
    sys.stdout.flush()


def test_inference_main_two_ranks_one_clip_writes_the_one_process_video(tmp_path, monkeypatch):
    import inference
    import viewcrafter
    tmp = str(tmp_path)
    open(os.path.join(tmp, "ckpt"), "w").write("x")
    torch.save(torch.full((3, 16, 16, 3), 0.3), os.path.join(tmp, "r0.pt"))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "VCX_GUIDANCE_PARALLEL", "VCX_CLIP_BATCH", "VCX_CLIPS_PER_GPU"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(viewcrafter, "build_diffusion_model", viewcrafter.build_diffusion_model)      # restored after the test
    monkeypatch.setattr(viewcrafter, "image_guided_synthesis", viewcrafter.image_guided_synthesis)
    _stub_entry(0, expect_group=False)
    inference.main(_argv(tmp, "one"))
    want = torch.load(os.path.join(tmp, "out", "one", "diffusion0.pt"))
    _spawn(_entry_worker, 2, (tmp,))
    got = torch.load(os.path.join(tmp, "out", "split", "diffusion0.pt"))
    assert torch.equal(got, want) and float(want.abs().max()) > 0.0
    lines = open(os.path.join(tmp, "stdout0.txt")).read().splitlines()
    assert "[guidance-parallel] 1 groups of 2: [[0, 1]], idle []" in lines
    other = open(os.path.join(tmp, "stdout1.txt")).read()
    assert "groups of" not in other and "[guidance-parallel] rank 1 group 0 position 1:" in other      # its own report only


# ------------------------------------------------------------------------------------------------------ 6. the single-view modes
_FAKE_SINGLE_VIEW = '''
import os
import torch
class ViewCrafter:
    def __init__(self, opts, gradio=False):
        self.opts = opts
        self.setup_diffusion()
    def nvs_single_view(self, gradio=False):
        here = os.path.dirname(__file__)
        open(os.path.join(here, "geometry_ran.rank" + os.environ.get("RANK", "0")), "w").close()
        if os.path.exists(os.path.join(here, "fail")):
            raise ValueError("dust3r exploded")
        jitter = torch.randn(3, 1, 1, 1)                    # the geometry stage draws from the global generator
        renders = (torch.full((3, 16, 16, 3), 0.4) + 0.01 * jitter).clamp(0, 1)
        out = self.run_diffusion(renders)
        with open(os.path.join(self.opts.save_dir, "diffusion0.mp4"), "wb") as f:
            f.write(b"placeholder")
        return out
'''


def _single_view_argv(tmp, exp):
    return ["--config", "none.yaml", "--ckpt_path", os.path.join(tmp, "ckpt"), "--out_dir", os.path.join(tmp, "out"), "--exp_name", exp,
            "--device", "cpu", "--video_length", "3", "--height", "16", "--width", "16", "--seed", "11",
            "--mode", "single_view_txt", "--reference_root", os.path.join(tmp, "ref")]


def _single_view_worker(rank, world, port, tmp, exp):
    _rank_env(rank, world, port)
    os.environ["VCX_GUIDANCE_PARALLEL"] = "1"
    import inference
    _stub_entry(rank, expect_group=True)
    res = dict(out=None, error=None)
    try:
        res["out"] = inference.main(_single_view_argv(tmp, exp))
    except RuntimeError as e:
        res["error"] = str(e)
    res["rng"] = torch.random.get_rng_state()
    torch.save(res, os.path.join(tmp, f"{exp}{rank}.pt"))


def test_single_view_mode_on_two_ranks_runs_geometry_once_and_writes_the_one_process_video(tmp_path, monkeypatch):
    """`--mode single_view_txt` with a stand-in reference checkout whose nvs_single_view draws random numbers, calls run_diffusion and
    writes a placeholder video (as the reference's does): geometry on rank 0 only, the same generator state on both ranks afterwards,
    rank 0's diffusion0.pt equal to the one-process run's result, the placeholder gone - and a failure of the geometry raised on both."""
    import inference
    import viewcrafter
    tmp = str(tmp_path)
    open(os.path.join(tmp, "ckpt"), "w").write("x")
    os.makedirs(os.path.join(tmp, "ref"))
    open(os.path.join(tmp, "ref", "viewcrafter.py"), "w").write(_FAKE_SINGLE_VIEW)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "VCX_GUIDANCE_PARALLEL", "VCX_CLIP_BATCH", "VCX_CLIPS_PER_GPU", "VIEWCRAFTER_REFERENCE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(viewcrafter, "build_diffusion_model", viewcrafter.build_diffusion_model)      # restored after the test
    monkeypatch.setattr(viewcrafter, "image_guided_synthesis", viewcrafter.image_guided_synthesis)
    _stub_entry(0, expect_group=False)
    want = inference.main(_single_view_argv(tmp, "one"))
    assert open(os.path.join(tmp, "out", "one", "diffusion0.mp4"), "rb").read() == b"placeholder"     # the stand-in's own writer
    # one process with the switch on is refused, as with --renderings, before the geometry runs
    os.remove(os.path.join(tmp, "ref", "geometry_ran.rank0"))
    monkeypatch.setenv("VCX_GUIDANCE_PARALLEL", "1")
    with pytest.raises(ValueError, match="needs at least 2 ranks"):
        inference.main(_single_view_argv(tmp, "refused"))
    assert not os.path.exists(os.path.join(tmp, "ref", "geometry_ran.rank0"))
    monkeypatch.delenv("VCX_GUIDANCE_PARALLEL")

    _spawn(_single_view_worker, 2, (tmp, "split"))
    got = [torch.load(os.path.join(tmp, f"split{r}.pt")) for r in range(2)]
    assert got[0]["error"] is None and got[1]["error"] is None, (got[0]["error"], got[1]["error"])
    ref = os.path.join(tmp, "ref")
    assert os.path.exists(os.path.join(ref, "geometry_ran.rank0")) and not os.path.exists(os.path.join(ref, "geometry_ran.rank1"))
    assert torch.equal(got[0]["rng"], got[1]["rng"]), "the ranks of the group do not continue from the same generator state"
    assert got[1]["out"] is None and torch.equal(got[0]["out"], want)
    out_dir = os.path.join(tmp, "out", "split")
    assert torch.equal(torch.load(os.path.join(out_dir, "diffusion0.pt")), want) and float(want.abs().max()) > 0.0
    videos = sorted(f for f in os.listdir(out_dir) if f.startswith("diffusion0.") and f != "diffusion0.pt")
    assert len(videos) == 1, videos
    assert open(os.path.join(out_dir, videos[0]), "rb").read() != b"placeholder"

    open(os.path.join(ref, "fail"), "w").close()
    _spawn(_single_view_worker, 2, (tmp, "failing"))
    for r in range(2):
        err = torch.load(os.path.join(tmp, f"failing{r}.pt"))["error"]
        assert err is not None and "rank 0 failed while producing the clips: ValueError: dust3r exploded" in err, (r, err)

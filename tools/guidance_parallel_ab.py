"""One video on several GPUs (VCX_GUIDANCE_PARALLEL, viewcrafter_amd/parallel.py): what a DDIM step costs by default and on one rank of
a guidance group.

    python tools/guidance_parallel_ab.py [--workloads ViewCrafter_25_576x1024x25,ViewCrafter_25_512_320x512x25] [--rounds 5] [--steps 3]
    python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 tools/guidance_parallel_ab.py   (3 ranks: --multicond)

One process (ONE GPU): a PROJECTION, not a speed-up - same box, same process, interleaved rounds, synthetic weights and conditioning:
  default        the product step: ONE stacked forward with the shared CFG prefix (2 videos with CFG, 3 with multi-condition
                 guidance) + the fused step kernel
  one rank       what a rank of a group executes: ONE B = 1 forward of one conditioning + the same step kernel (the other ranks'
                 outputs are stand-in tensors: no exchange is timed)
The ratio is the ceiling of the speed-up of a group BEFORE the cost of the exchange (one all_gather of an fp32 v per step).  The shared
prefix is lost on the split route, so the ceiling is below the number of ranks.
Several processes (>= 2 GPUs, RCCL): the real thing - every rank times the split step including the exchange; rank 0 also times the
default step on its GPU and prints the measured ratio."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _StandIn:
    """The other ranks' denoiser outputs as fixed tensors: the one-GPU projection times no exchange."""

    def __init__(self, size, position=0):
        self.size, self.position, self.index, self.others = size, position, 0, None

    def exchange(self, v):
        if self.others is None:
            self.others = [torch.randn_like(v) for _ in range(self.size)]
        return [v if i == self.position else self.others[i] for i in range(self.size)]

    def check_equal(self, x, **kw):
        pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="ViewCrafter_25_576x1024x25,ViewCrafter_25_512_320x512x25")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--multicond", action="store_true", help="several processes: groups of 3 (multi-condition guidance)")
    args = ap.parse_args()
    from bench import WORKLOADS, synth_conditioning
    from tools.telemetry import Telemetry
    from viewcrafter_amd import parallel
    from viewcrafter_amd.builder import build_diffusion_model, randomize_parameters
    from viewcrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    from viewcrafter_amd.lvdm.models.samplers.ddim_multiplecond import DDIMSampler as DDIMSamplerMulti
    rank, world = parallel.init_distributed()
    device = f"cuda:{parallel.local_device_index()}" if world > 1 else "cuda"
    real = parallel.build_guidance_group(3 if args.multicond else 2) if world > 1 else None

    for workload in args.workloads.split(","):
        cfg, T, h, w = WORKLOADS[workload]
        model = build_diffusion_model(os.path.join(ROOT, "configs", cfg), device=device, conditioners="identity")
        randomize_parameters(model)
        x, cond, uc = synth_conditioning(T, h, w, device, seed=123)
        ctx, uctx = cond["c_crossattn"][0], uc["c_crossattn"][0]
        uc2 = {"c_crossattn": [torch.cat([uctx[:, :77], ctx[:, 77:]], 1)], "c_concat": cond["c_concat"]}
        fs = torch.tensor([10], device=device)

        def make(multi, group):
            s = (DDIMSamplerMulti if multi else DDIMSampler)(model)
            s.make_schedule(ddim_num_steps=50, ddim_discretize="uniform_trailing", ddim_eta=1.0, verbose=False)
            s.guidance_group = group
            kw = dict(cfg_img=3.0, unconditional_conditioning_img_nonetext=uc2) if multi else {}

            def go(index=25):
                y = x
                t = torch.full((1,), int(s.ddim_timesteps[index]), device=device, dtype=torch.long)
                for _ in range(args.steps):
                    y = s.p_sample_ddim(y, cond, t, index=index, unconditional_guidance_scale=7.5, unconditional_conditioning=uc, fs=fs,
                                        guidance_rescale=0.7, **kw)[0]
                return y
            return go
        if real is None:
            runs = {"CFG default (B = 2, shared prefix)": make(False, None), "CFG one rank (B = 1)": make(False, _StandIn(2)),
                    "multi-condition default (B = 3, shared prefix)": make(True, None),
                    "multi-condition one rank (B = 1)": make(True, _StandIn(3))}
        else:
            runs = {"split step incl. exchange": make(args.multicond, real) if real.position is not None else (lambda: None)}
            if rank == 0:
                runs["default step on rank 0's GPU"] = make(args.multicond, None)
        times, tele = {n: [] for n in runs}, {n: [] for n in runs}
        with torch.no_grad():
            for name, fn in runs.items():
                fn()                   # warm-up: weight packs, context K / V, communicator
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for name, fn in runs.items():
                    if real is not None and name.startswith("split"):
                        torch.distributed.barrier()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with Telemetry(device_index=torch.cuda.current_device(), period_s=0.05) as tm:
                        e0.record()
                        fn()
                        e1.record()
                        torch.cuda.synchronize()
                    times[name].append(e0.elapsed_time(e1) / args.steps)
                    tele[name].append(tm.summary())
        med = {n: sorted(v)[len(v) // 2] for n, v in times.items()}
        if rank == 0:
            kind = "ONE-GPU PROJECTION (no exchange, no second GPU)" if real is None else f"{world} ranks, backend {torch.distributed.get_backend()}"
            print(f"{workload}: ms per DDIM step, median of {args.rounds} interleaved rounds of {args.steps} steps - {kind}")
            print("| step | ms (median) | all rounds | sclk MHz (mean) |")
            print("|---|---|---|---|")
            for name in runs:
                sclk = [s["sclk_mhz"]["mean"] for s in tele[name] if s.get("source") and s.get("sclk_mhz")]
                print(f"| {name} | {med[name]:.2f} | {[round(t, 2) for t in times[name]]} | {sum(sclk) / len(sclk):.0f} |" if sclk else
                      f"| {name} | {med[name]:.2f} | {[round(t, 2) for t in times[name]]} | n/a |")
            names = list(runs)
            if real is None:
                print(f"projected ceiling before exchange cost: CFG {med[names[0]] / med[names[1]]:.3f}x on 2 GPUs, "
                      f"multi-condition {med[names[2]] / med[names[3]]:.3f}x on 3 GPUs")
            else:
                print(f"measured: default {med[names[1]]:.2f} ms / split {med[names[0]]:.2f} ms = {med[names[1]] / med[names[0]]:.3f}x")
        del model
        torch.cuda.empty_cache()
    parallel.shutdown()


if __name__ == "__main__":
    main()

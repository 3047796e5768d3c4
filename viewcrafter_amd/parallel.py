"""Trajectory sharding across the GPUs of one node (one process per GPU, torch.distributed on RCCL over xGMI).

The unit of work on this path is one trajectory / clip = one `image_guided_synthesis` call: independent noise and
conditioning, no cross-sample operation anywhere in the UNet, the VAE or the sampler.  So the DDIM loop
needs NO in-step collective; the only communication is
  (i)  once at start-up: broadcast of the weights from rank 0 (2.9 GB fp16 / 5.8 GB fp32; instead of N disk reads) and
       of any conditioning the trajectories share,
  (ii) once at the end: gather of the decoded clips (or of timing scalars) to rank 0.
Rank r takes trajectories r, r + W, r + 2W, ...  The reference has no multi-GPU inference at all; its only collective
helper is the dead `gather_data` (lvdm/common.py:8-14), kept there for API parity.

VCX_GUIDANCE_PARALLEL=1 (opt-in; `guidance_layout`, `GuidanceGroup`): ONE trajectory on several GPUs.  Every DDIM step evaluates the
denoiser on the same x / t / fs / c_concat under 2 (CFG) or 3 (multi-condition) conditionings; consecutive ranks form a group of that
size, each rank evaluates the conditioning of its position and one all_gather of the fp32 `v` per step (3.7 MB at 25 x 72 x 128) gives
every rank of the group all of them.  The step kernel then runs redundantly on every rank, so x never travels.  Clips are sharded over
the groups, the results gathered over the groups' first ranks (the leaders).
"""
import os

import torch
import torch.distributed as dist


def init_distributed(backend=None):
    """Initialise from the torchrun environment.  backend: 'nccl' (= RCCL on ROCm) on GPUs, 'gloo' on CPU."""
    if dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world == 1:
        return 0, 1
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC only on this driver
    if backend is None:
        backend = os.environ.get("VCX_DIST_BACKEND", "").strip().lower() or None
        if backend not in (None, "gloo", "nccl"):
            raise ValueError(f"VCX_DIST_BACKEND must be gloo or nccl, got {backend!r}")
    if backend is None:
        backend = "nccl" if torch.cuda.is_available() else "gloo"
    kw = {}
    if backend == "nccl":
        local = local_device_index()
        torch.cuda.set_device(local)
        kw["device_id"] = torch.device("cuda", local)
    dist.init_process_group(backend, **kw)
    return dist.get_rank(), dist.get_world_size()


def local_device_index():
    """The GPU of this rank: LOCAL_RANK.  VCX_SHARE_GPU=1 (a TEST mode, not a way to run: the GPU suite places two or three ranks on
    its one GPU with a gloo control plane - RCCL refuses two ranks on one device) wraps it round the devices present."""
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("VCX_SHARE_GPU") == "1" and torch.cuda.is_available():
        local %= max(1, torch.cuda.device_count())
    return local


def rank_world():
    """(rank, world size) of the current process group, (0, 1) without one."""
    return (dist.get_rank(), dist.get_world_size()) if dist.is_initialized() else (0, 1)


def shard_indices(n_items, rank, world):
    """Round-robin ownership: rank r owns items r, r+W, ...  (balanced to within one item)."""
    return list(range(rank, n_items, world))


def owner_of(index, world):
    return index % world


@torch.no_grad()
def broadcast_module_(module, src=0, bucket_bytes=256 << 20, _force=False):
    """Make every rank's parameters and buffers equal to rank `src`'s with a few large broadcasts (xGMI is
    point-to-point: few big messages beat thousands of small ones).  Tensors are grouped by (dtype, device) into flat
    buckets; under RCCL a tensor that lives on the host is staged through the current GPU.
    `_force`: run the collectives even in a one-rank group (tests/test_entry_gpu.py exercises the RCCL path on one GPU)."""
    if not dist.is_initialized() or (dist.get_world_size() == 1 and not _force):
        return module
    rccl = dist.get_backend() == "nccl"
    tensors = [p.data for p in module.parameters()] + [b.data for b in module.buffers()]
    groups = {}
    for t in tensors:
        groups.setdefault((t.dtype, t.device), []).append(t)
    for (dtype, device), group in groups.items():
        staged = rccl and device.type != "cuda"
        to_host = not rccl and device.type == "cuda"         # gloo control plane with the model on a GPU (VCX_SHARE_GPU test mode)
        bucket, size = [], 0
        for t in group + [None]:
            if t is not None and (size + t.numel() * t.element_size() <= bucket_bytes or not bucket):
                bucket.append(t)
                size += t.numel() * t.element_size()
                continue
            flat = torch.cat([b.reshape(-1) for b in bucket])
            if staged:
                flat = flat.cuda()
            elif to_host:
                flat = flat.cpu()
            dist.broadcast(flat, src=src)
            if staged or to_host:
                flat = flat.to(device)
            off = 0
            for b in bucket:
                b.copy_(flat[off:off + b.numel()].view_as(b))
                off += b.numel()
            bucket, size = ([t], t.numel() * t.element_size()) if t is not None else ([], 0)
    drop_packed_copies(module)
    return module


def drop_packed_copies(module):
    """Parameters were overwritten in place: every PackedModule below `module` (the root usually is a plain nn.Module)
    must forget its kernel-layout fp16 copies, and the UNet its cached context K/V and captured graphs."""
    for m in module.modules():
        if hasattr(m, "_drop_packed"):
            m._drop_packed()
    return module


def broadcast_tensor(t, src=0):
    if dist.is_initialized() and dist.get_world_size() > 1:
        dist.broadcast(t, src=src)
    return t


def broadcast_tensor_list(tensors, src=0, error=None):
    """Rank `src` holds a list of tensors (any shapes / dtypes), the others pass None: afterwards every rank holds the list.
    The shapes travel first as one small object broadcast, the payload as one dist.broadcast per tensor (on the GPU under RCCL,
    on the host under gloo).  `error` (rank src only): a failure that happened while PRODUCING the list - it is broadcast in place
    of the metadata and raised on every rank together, so that nobody waits in a collective the source never joins."""
    if not dist.is_initialized() or dist.get_world_size() == 1:
        if error is not None:
            raise RuntimeError(error)
        return list(tensors)
    rank = dist.get_rank()
    meta = [None]
    if rank == src:
        meta = [("error", str(error)) if error is not None else
                ("ok", [(tuple(t.shape), str(t.dtype).replace("torch.", "")) for t in tensors])]
    dist.broadcast_object_list(meta, src=src)
    kind, info = meta[0]
    if kind == "error":
        raise RuntimeError(f"rank {src} failed while producing the clips: {info}")
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
    out = []
    for i, (shape, dtype) in enumerate(info):
        t = tensors[i].to(dev).contiguous() if rank == src else torch.empty(shape, dtype=getattr(torch, dtype), device=dev)
        dist.broadcast(t, src=src)
        out.append(tensors[i] if rank == src else t)
    return out


def broadcast_rng_state(src=0):
    """Every rank's global generators (CPU, and the current GPU's when there is one) continue from rank `src`'s state."""
    if not dist.is_initialized() or dist.get_world_size() == 1:
        return
    cuda = torch.cuda.is_available()
    state = [None]
    if dist.get_rank() == src:
        state = [(torch.random.get_rng_state(), torch.cuda.get_rng_state().cpu() if cuda else None)]
    dist.broadcast_object_list(state, src=src)
    cpu_state, cuda_state = state[0]
    torch.random.set_rng_state(cpu_state)
    if cuda and cuda_state is not None:
        torch.cuda.set_rng_state(cuda_state)


def gather_results(local, n_items, dst=0, _force=False, group=None):
    """local: {item index: tensor} owned by this rank (all tensors of one shape/dtype).  Returns on rank `dst` the list
    of all n_items results in item order (None elsewhere).  One all_gather of a padded stack per call.
    (`_force`: as in broadcast_module_.)  `group`: a GuidanceGroup - the items are owned by GROUPS, every rank of a group holds the
    same results, and the gather runs over the groups' leaders only (every other rank returns None at once)."""
    if not dist.is_initialized() or (dist.get_world_size() == 1 and not _force):
        return [local[i] for i in range(n_items)]
    if group is not None:
        if group.position != 0:
            return None
        rank, world, pg = group.index, group.n_groups, group.leaders
        if world == 1:
            return [local[i] for i in range(n_items)]
    else:
        rank, world, pg = dist.get_rank(), dist.get_world_size(), None
    if n_items == 0:
        return [] if rank == dst else None
    per_rank = (n_items + world - 1) // world
    example = next(iter(local.values())) if local else None
    # every rank reports the (shape, dtype) of ALL its results first: a mismatch must fail on every rank together - if only the
    # rank holding the odd clip raised, the others would wait in the all_gather below until the launcher kills them
    mine = sorted({(tuple(t.shape), str(t.dtype).replace("torch.", "")) for t in local.values()})
    meta = [None] * world
    dist.all_gather_object(meta, mine, group=pg)
    kinds = sorted({k for m in meta for k in m})
    if len(kinds) != 1:
        raise ValueError(f"gather_results needs results of one shape and dtype, the ranks hold {kinds} "
                         "(clips of different length / size must be generated in separate launches)")
    shape, dtype = kinds[0]
    rccl = dist.get_backend() == "nccl"
    dev = example.device if example is not None else (torch.device("cuda", torch.cuda.current_device())
                                                      if rccl else torch.device("cpu"))
    if group is not None and not rccl:
        dev = torch.device("cpu")       # the leaders' gather under gloo takes host tensors (results on a GPU are staged: VCX_SHARE_GPU
                                        # test mode); without a group nothing changes
    stack = torch.zeros((per_rank,) + tuple(shape), dtype=getattr(torch, dtype), device=dev)
    for slot, idx in enumerate(shard_indices(n_items, rank, world)):
        stack[slot] = local[idx]
    out = [torch.empty_like(stack) for _ in range(world)]
    dist.all_gather(out, stack, group=pg)
    if rank != dst:
        return None
    return [out[owner_of(i, world)][i // world] for i in range(n_items)]


def _owner_rank_world(group):
    """(rank, world) that own items: the process's rank among all ranks, or its GROUP among the groups (group: a GuidanceGroup; an idle
    rank owns nothing)."""
    if group is not None:
        return group.index, group.n_groups
    return (dist.get_rank(), dist.get_world_size()) if dist.is_initialized() else (0, 1)


def run_sharded(fn, items, gather=True, lanes=1, model=None, group=None):
    """Apply fn(item, index) to the items this rank owns; optionally gather the tensor results on rank 0.  lanes > 1: that many of the
    rank's items in flight at a time, interleaved step by step on their own HIP streams (interleave.run_interleaved); `model`: the
    module the lanes share - its lazily built weight packs are built here, on the caller's stream, before the lanes start.
    `group` (a GuidanceGroup, default None = unchanged): the items are sharded over the guidance groups, not the ranks - every rank of
    group g runs items g, g + G, ..."""
    rank, world = _owner_rank_world(group)
    mine = [] if rank is None else list(shard_indices(len(items), rank, world))
    if lanes > 1 and len(mine) > 1:
        from .interleave import prepack, run_interleaved
        if model is not None and torch.cuda.is_available():
            prepack(model)
        local = dict(zip(mine, run_interleaved(fn, [(i, items[i]) for i in mine], n_lanes=lanes)))
    else:
        local = {i: fn(items[i], i) for i in mine}
    return gather_results(local, len(items), group=group) if gather else local


def run_sharded_batched(fn, items, clip_batch, gather=True, group=None):
    """run_sharded for a function of several items at once: fn(list of items, list of their indices) -> list of results.  The items this
    rank owns go to fn `clip_batch` at a time, in order (the last group may be smaller; VCX_CLIP_BATCH, clip_batch.py).  `group`: as in
    run_sharded."""
    from .clip_batch import groups
    rank, world = _owner_rank_world(group)
    local = {}
    for part in groups([] if rank is None else shard_indices(len(items), rank, world), max(1, int(clip_batch))):
        outs = fn([items[i] for i in part], part)
        if len(outs) != len(part):
            raise ValueError(f"run_sharded_batched: {len(outs)} results for {len(part)} items")
        local.update(zip(part, outs))
    return gather_results(local, len(items), group=group) if gather else local


# ---------------------------------------------------------------------------------------------- one video on several GPUs
def guidance_parallel_from_env(environ=None):
    """VCX_GUIDANCE_PARALLEL: unset / empty / 0 = off (the default), 1 = the guidance evaluations of one video are split over the ranks of
    a group.  Refuses VCX_CLIPS_PER_GPU > 1 beside it: two lanes issuing collectives on two streams is a hazard not worth owning."""
    env = os.environ if environ is None else environ
    raw = env.get("VCX_GUIDANCE_PARALLEL", "0").strip() or "0"
    if raw not in ("0", "1"):
        raise ValueError(f"VCX_GUIDANCE_PARALLEL must be 0 or 1, got {raw!r}")
    if raw == "0":
        return False
    try:
        lanes = int(env.get("VCX_CLIPS_PER_GPU", "1"))
    except ValueError:
        lanes = 1
    if lanes > 1:
        raise ValueError(f"VCX_GUIDANCE_PARALLEL=1 and VCX_CLIPS_PER_GPU={lanes} cannot be combined: the lanes would issue the per-step "
                         "exchange on two streams")
    return True


def guidance_layout(world, copies):
    """Ranks of a guidance-parallel launch: (n_groups, group_of_rank, position_of_rank, idle_ranks).  `copies` = denoiser evaluations per
    step (clip_batch.guidance_copies: 2 with CFG, 3 with multi-condition guidance).  Group g is the consecutive ranks
    [g * copies, (g + 1) * copies) - neighbouring GPUs; the ranks beyond n_groups * copies are idle (None in both lists)."""
    world, copies = int(world), int(copies)
    if copies <= 1:
        raise ValueError("guidance-parallel sampling has nothing to split: with guidance scale 1.0 a step is ONE denoiser evaluation")
    if world < copies:
        raise ValueError(f"guidance-parallel sampling needs at least {copies} ranks (one per guidance evaluation), the launch has {world}")
    n_groups = world // copies
    used = n_groups * copies
    group_of_rank = [r // copies if r < used else None for r in range(world)]
    position_of_rank = [r % copies if r < used else None for r in range(world)]
    return n_groups, group_of_rank, position_of_rank, list(range(used, world))


def _host_staged(pg):
    return dist.get_backend(pg) != "nccl"


class GuidanceGroup:
    """The ranks that share one video's guidance evaluations.  size: ranks in the group (= guidance copies); position: this rank's place
    in it (= which conditioning it evaluates; None on an idle rank); index: the group's number (owns clips index, index + G, ...);
    group: its process group; n_groups / leaders: the number of groups and the process group of their position-0 ranks (result gather);
    ranks: the global ranks of this group."""

    def __init__(self, size, position, index, group, n_groups=1, leaders=None, ranks=None, idle=()):
        self.size, self.position, self.index, self.group = size, position, index, group
        self.n_groups, self.leaders, self.idle = n_groups, leaders, list(idle)
        self.ranks = list(ranks) if ranks is not None else list(range(size))
        self._buf = self._host = None
        # what this rank did on the split route, counted where it happens (sampler: steps, forwards; here: exchanges) - report()
        self.stats = dict(steps=0, forwards=0, exchanges=0, batch=None)

    def _buffers(self, v):
        shape = (self.size,) + tuple(v.shape)
        if self._buf is None or tuple(self._buf.shape) != shape or self._buf.dtype != v.dtype or self._buf.device != v.device:
            self._buf = torch.empty(shape, dtype=v.dtype, device=v.device)
            self._host = None
            if _host_staged(self.group) and v.device.type != "cpu":
                self._host = torch.empty(shape, dtype=v.dtype)
        return self._buf, self._host

    def exchange(self, v_local):
        """Every rank passes the denoiser output of ITS conditioning; returns the `size` outputs in position order.  They are VIEWS of
        one buffer [size, *v.shape] that is reused as long as the shapes stay the same (a whole sample() call and the next): the next
        exchange overwrites them, so read them first (the step kernel does) and clone what must outlive the step.  One
        all_gather_into_tensor: under RCCL it is enqueued on the process group's own stream, ordered after the current stream's work
        and before its later work by events, with no host synchronisation; under gloo it is staged through the host."""
        self.stats["exchanges"] += 1
        v = v_local.contiguous()
        buf, host = self._buffers(v)
        if host is not None:            # (flat views: every backend takes the concatenation of 1-D tensors)
            dist.all_gather_into_tensor(host.view(-1), v.reshape(-1).cpu(), group=self.group)
            buf.copy_(host)
        else:
            dist.all_gather_into_tensor(buf.view(-1), v.view(-1), group=self.group)
        return [buf[i] for i in range(self.size)]

    def report(self, rank):
        """One line per rank at the end of a guidance-parallel run: what THIS rank executed on the split route."""
        st = self.stats
        return (f"[guidance-parallel] rank {rank} group {self.index} position {self.position}: {st['steps']} steps, {st['forwards']} "
                f"forwards of batch {st['batch']} under its own conditioning, {st['exchanges']} exchanges")

    @staticmethod
    def checksum(x):
        """An exact checksum of a tensor's bits (the int64 sum of its 32- or 16-bit patterns) as a one-element tensor on x's device;
        no host synchronisation."""
        bits = x.detach().contiguous().view(torch.int32 if x.element_size() == 4 else torch.int16)
        return bits.to(torch.int64).sum().reshape(1)

    def check_equal(self, x, what="the final latent", also=None):
        """The ranks of a group never send x: they hold the same x_T and draw the same noise, so it stays bit-equal - CHECKED here, once
        per video: the checksum of x (and `also`: {name: checksum taken earlier}, e.g. of x_T - a deviation there can be rounded away
        by the end of the loop), ONE small all_gather, one host sync.  A mismatch raises on every rank of the group together."""
        names = [what] + list(also or {})
        mine = torch.cat([self.checksum(x)] + [c.reshape(1) for c in (also or {}).values()])
        if _host_staged(self.group):
            mine = mine.cpu()
        every = torch.empty(self.size * len(names), dtype=torch.int64, device=mine.device)
        dist.all_gather_into_tensor(every, mine, group=self.group)
        sums = every.view(self.size, len(names)).tolist()
        for j, name in enumerate(names):
            col = [row[j] for row in sums]
            if len(set(col)) != 1:
                odd = [r for r, c in zip(self.ranks, col) if c != col[0]]
                raise RuntimeError(f"guidance-parallel group {self.index} (ranks {self.ranks}): {name} differs between the ranks - ranks "
                                   f"{odd} do not hold the bits of rank {self.ranks[0]} (checksums {dict(zip(self.ranks, col))}); the "
                                   "ranks of a group must start from the same seed and draw the same noise")


def build_guidance_group(copies):
    """The GuidanceGroup of this rank in the current launch.  EVERY rank creates EVERY group (dist.new_group is collective over the
    world) in the same order, then the group of the leaders."""
    rank, world = rank_world()
    n_groups, group_of_rank, position_of_rank, idle = guidance_layout(world, copies)
    mine = None
    for g in range(n_groups):
        pg = dist.new_group(list(range(g * copies, (g + 1) * copies)))
        if group_of_rank[rank] == g:
            mine = pg
    leaders = dist.new_group([g * copies for g in range(n_groups)])
    g = group_of_rank[rank]
    return GuidanceGroup(copies, position_of_rank[rank], g, mine, n_groups=n_groups, leaders=leaders,
                         ranks=[] if g is None else range(g * copies, (g + 1) * copies), idle=idle)


def describe_layout(world, copies):
    """The one line rank 0 prints at the start of a guidance-parallel launch."""
    n_groups, _, _, idle = guidance_layout(world, copies)
    groups = [list(range(g * copies, (g + 1) * copies)) for g in range(n_groups)]
    return f"[guidance-parallel] {n_groups} groups of {copies}: {groups}, idle {idle}"


def shutdown(barrier=True):
    """(Barrier +) destroy_process_group when a group exists (end of a torchrun launch)."""
    if dist.is_initialized():
        try:
            if barrier:
                dist.barrier()
        finally:
            dist.destroy_process_group()

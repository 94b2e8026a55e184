"""The weight keeper: a model's parameters in ONE fp32 arena plus every kernel-side copy of them, and the host arithmetic that lays both out.

Two halves:
  * planning — plain functions over shapes and offsets (Python / numpy, no device allocation): the arena order and offsets, the transposed
    tiles, the fragment and remainder chunk indices, the remainder segments and ranges, the conv repack rows; `plan_arena` runs them all.
  * `WeightKeeper` — allocates what a plan describes, registers the views with hulc2_amd.shadow and keeps the copies fresh: what an
    EXTERNAL optimizer loop needs (Lightning + torch.optim / hulc2_amd.optim, hulc2/training.py:79-82) and what the native loop
    (trainer.ArenaTrainer, a subclass) builds on.
"""
from types import SimpleNamespace
from typing import List, Optional, Tuple

import weakref

import numpy as np
import torch

from . import gradsink
from . import kernels as kn
from . import shadow
from . import switches

MAX_KERNEL_RANGES = 8              # element ranges an optimizer kernel takes (remainder ranges, skip ranges)


# ---- intervals ---------------------------------------------------------------------------------------------------------------------------
def merge_ranges(ranges, gap: int = 0) -> List[Tuple[int, int]]:
    """sorted, disjoint (begin, end) ranges covering the given ones; neighbours at most `gap` elements apart become one (0: touching and
    overlapping ranges only)"""
    merged = []
    for a, b in sorted(ranges):
        if merged and a - merged[-1][1] <= gap:
            merged[-1][1] = max(merged[-1][1], b)
        else:
            merged.append([a, b])
    return [(a, b) for a, b in merged]


def close_to(ranges, limit: int) -> List[Tuple[int, int]]:
    """at most `limit` ranges: the smallest gaps are closed first (what lies in a closed gap is covered too)"""
    merged = [list(r) for r in merge_ranges(ranges)]
    while len(merged) > limit:
        i = min(range(len(merged) - 1), key=lambda k: merged[k + 1][0] - merged[k][1])
        merged[i][1] = merged[i + 1][1]
        del merged[i + 1]
    return [(a, b) for a, b in merged]


def span_ranges(offsets, total: int, indices) -> List[Tuple[int, int]]:
    """merged arena ranges of the parameters with these indices: a parameter's span runs up to its successor's offset (the alignment padding
    behind it is zero and stays zero)"""
    ends = list(offsets[1:]) + [total]
    return merge_ranges((offsets[i], ends[i]) for i in indices)


# ---- the plan ----------------------------------------------------------------------------------------------------------------------------
def fused_groups(model) -> list:
    """(module, group) for every group of parameters a module wants back to back in the arena (fused_param_groups: the decoder's four heads
    become one (184, H) matrix view), all members trainable"""
    return [(mod, g) for mod in model.modules() if getattr(mod, "fused_param_groups", None) is not None
            for g in mod.fused_param_groups() if all(p.requires_grad for p in g["params"])]


def plan_order(params, groups):
    """arena order = registration order, except that the members of a group follow its first member.  Ungrouped parameters are padded to 8
    elements (16-byte alignment in both the fp32 and the bf16 arena); members are tightly packed, then comes the group's zero padding.
    Returns (ordered parameters, offsets, total, {group index: offset})."""
    member = {id(p): gi for gi, (_, g) in enumerate(groups) for p in g["params"]}
    order, placed = [], set()
    for p in params:
        gi = member.get(id(p))
        if gi is None:
            order.append((p, None))
        elif gi not in placed:
            placed.add(gi)
            order += [(q, gi) for q in groups[gi][1]["params"]]
    offsets, total, group_spans = [], 0, {}
    for i, (p, gi) in enumerate(order):
        offsets.append(total)
        if gi is None:
            total += (p.numel() + 7) // 8 * 8
            continue
        group_spans.setdefault(gi, total)
        total += p.numel()
        if i + 1 == len(order) or order[i + 1][1] != gi:
            total = (total + groups[gi][1]["pad"] + 7) // 8 * 8
    return [p for p, _ in order], offsets, total, group_spans


def plan_tiles(params, offsets, names, member, groups, group_spans):
    """transposed bf16 shadows of the nn.Linear weights (data-gradient GEMMs read W^T k-major); RNN and conv weights are consumed in place by
    their own kernels and stay out of the table, as do matrices too thin to tile and the members of a fused group (the group is one matrix).
    Returns (matrices [(parameter | group index, offset, (rows, cols))], int64 (n, 5) {offset, rows, cols, tile row, tile col})."""
    mats = []
    for p, off in zip(params, offsets):
        nm = names.get(id(p), "")
        if p.dim() != 2 or "rnn.weight_hh" in nm or "rnn.weight_ih_l1" in nm or "birnn_model.weight_hh" in nm or min(p.shape) < 8 or id(p) in member:
            continue
        mats.append((p, off, tuple(p.shape)))
    mats += [(gi, group_spans[gi], tuple(g["shape"])) for gi, (_, g) in enumerate(groups) if len(g["shape"]) == 2]
    tiles = [(off, r, c, i, j) for _, off, (r, c) in mats for i in range((r + 63) // 64) for j in range((c + 63) // 64)]
    return mats, np.array(tiles, dtype=np.int64).reshape(-1, 5)


def _chunk_index(p, layout: int, off: int) -> np.ndarray:
    """source 8-byte chunks (arena elements / 4) of one weight in fragment layout `layout` (kernels.ffn_frag_perm)"""
    ff = p.shape[0] if layout in (0, 3) else p.shape[1]
    perm = kn.ffn_frag_perm(layout, ff).astype("int64").reshape(-1, 4)
    assert (perm[:, 0] % 4 == 0).all() and (perm[:, 1:] - perm[:, :1] == [1, 2, 3]).all(), "fragment permutations move runs of 4"
    return (perm[:, 0] + off) // 4


def _index_table(entries):
    """[(parameter, layout name, source chunks)] -> (int32 gather index, [(parameter, layout name, destination offset, elements)], length)"""
    views, dst = [], 0
    for p, name, _ in entries:
        views.append((p, name, dst, p.numel()))
        dst += p.numel()
    idx = np.concatenate([c for _, _, c in entries]).astype(np.uint32).view(np.int32) if entries else None
    return idx, views, dst


def _placed(modules, hook, off_of, member):
    """(parameter, what the hook says of it, arena offset) for the operands the kernels can read in place: in the arena, at a multiple of 4
    elements (an 8-byte chunk), no member of a fused group"""
    for m in modules:
        for p, what in (getattr(m, hook)() if hasattr(m, hook) else ()):
            off = off_of.get(id(p))
            if off is not None and off % 4 == 0 and id(p) not in member:
                yield p, what, off


def plan_frag(modules, off_of, member):
    """fragment-packed feed-forward weights of the transformer block launch (modules list them in frag_operands()): one gather launch per step
    from the bf16 arena and — bit 31 of the index, layouts 2 and 3 — its transposed shadow, 8-byte chunks"""
    return _index_table([(p, "ffn_p%d" % n, _chunk_index(p, n, off) | ((1 << 31) if n in (2, 3) else 0))
                         for p, n, off in _placed(modules, "frag_operands", off_of, member)])


def plan_lo(modules, off_of, member, total: int):
    """rounding remainders w - bf16(w) of the weights a split-operand forward reads (modules list them in lo_operands(): natural layout "lo" /
    "oihw_flat_lo", packed "ffn_p0_lo" / "ffn_p1_lo"): a second shadow arena at the bf16 shadow's offsets, which the optimizer kernels fill
    inside at most 8 element ranges while the new weights are in their registers.
    Returns (natural [(parameter, offset)], int64 (n, 3) segments {source offset, count, destination offset}, ranges, packed index table)."""
    nat, packed = {}, []
    for p, layout, off in _placed(modules, "lo_operands", off_of, member):
        nat.setdefault(id(p), (p, off))
        if layout not in ("lo", "oihw_flat_lo"):
            packed.append((p, layout, _chunk_index(p, int(layout[5]), off)))
    segs = [(off, p.numel(), off) for p, off in nat.values()]
    # (offsets are multiples of 8: the padding is the slice's own; remainders of the weights in a closed gap are written too: harmless)
    ranges = close_to([(a, a + (n + 3) // 4 * 4) for a, n, _ in segs], MAX_KERNEL_RANGES)
    return list(nat.values()), np.array(segs, dtype=np.int64).reshape(-1, 3), [(a, min(b, total)) for a, b in ranges], _index_table(packed)


def plan_conv(params, offsets, modules):
    """conv weights in their kernel layouts (OIHW flat for conv1, OHWI forward, IHWO data gradient), and Linears behind nn.Flatten of a
    (C, H, W) map (gripper encoder, flatten_linears()) in NHWC column order: one repack launch per step.
    Returns (int64 (n, 7) {source offset, destination offset, Cout, Cin, KH, KW, mode}, [(parameter, layout name, offset, shape)], length)."""
    flat_lin = {id(w): chw for m in modules if hasattr(m, "flatten_linears") for w, chw in m.flatten_linears()}
    rows, views, dst = [], [], 0
    for p, off in zip(params, offsets):
        chw = flat_lin.get(id(p))
        if p.dim() == 2 and chw is not None:
            co, (ci, kh, kw) = p.shape[0], chw
            modes = [("hwc", 1, (co, kh * kw * ci)), ("hwc_t", 3, (kh * kw * ci, co))]
        elif p.dim() != 4:
            continue
        else:
            co, ci, kh, kw = p.shape
            modes = [("oihw_flat", 0, (co, ci * kh * kw))] if ci < 8 else [("ohwi", 1, (co, kh * kw * ci)), ("ihwo", 2, (ci, kh, kw, co))]
        for name, mode, shape in modes:
            rows.append((off, dst, co, ci, kh, kw, mode))
            views.append((p, name, dst, shape))
            dst += (p.numel() + 7) // 8 * 8
    return np.array(rows, dtype=np.int64).reshape(-1, 7), views, dst


def plan_arena(model, fuse: bool) -> SimpleNamespace:
    """Everything the keeper allocates, as host data.  fuse: lay fused groups out back to back (their views receive their gradient through a
    sink only, so they exist only where sinks do)."""
    p = SimpleNamespace(groups=fused_groups(model) if fuse else [])
    p.member = {id(q) for _, g in p.groups for q in g["params"]}
    p.params, p.offsets, p.total, p.group_spans = plan_order([q for q in model.parameters() if q.requires_grad], p.groups)
    names = {id(q): n for n, q in model.named_parameters()}
    off_of = {id(q): off for q, off in zip(p.params, p.offsets)}
    modules = list(model.modules())
    p.mats, p.tiles = plan_tiles(p.params, p.offsets, names, p.member, p.groups, p.group_spans)
    # (the packed fragments read the transposed shadow: none without it)
    p.frag_idx, p.frag_views, p.frag_len = plan_frag(modules if len(p.tiles) else (), off_of, p.member)
    p.lo_nat, p.lo_seg, p.lo_ranges, (p.lo_frag_idx, p.lo_frag_views, p.lo_frag_len) = plan_lo(modules, off_of, p.member, p.total)
    p.conv_table, p.conv_views, p.conv_len = plan_conv(p.params, p.offsets, modules)
    return p


# ---- the keeper --------------------------------------------------------------------------------------------------------------------------
# parameter arenas by the address of their storage (weak: an arena lives as long as its trainer / the model's keeper)
_ARENAS: "weakref.WeakValueDictionary[int, WeightKeeper]" = weakref.WeakValueDictionary()


def arena_of(params) -> "Optional[WeightKeeper]":
    """the keeper whose fp32 arena holds exactly these parameters (same objects, every one a view of the arena), else None"""
    params = list(params)
    if not params or params[0].device.type != "cuda":
        return None
    tr = _ARENAS.get(params[0].untyped_storage().data_ptr())
    if tr is None or len(params) != len(tr.params):
        return None
    mine = {id(p) for p in tr.params}
    base = tr.flat_p.data_ptr()
    for p in params:
        if id(p) not in mine:
            return None
    for p, off in zip(tr.params, tr.offsets):
        if p.data_ptr() != base + off * 4 or p.dtype != torch.float32:
            return None
    return tr


class _LoadHook:
    """load_state_dict post-hook of a model with a keeper: re-derive the kernel-side copies (WeightKeeper._after_model_load)"""

    def __init__(self, keeper):
        self.ref = weakref.ref(keeper)

    def __call__(self, module, incompatible_keys):
        tr = self.ref()
        if tr is not None and tr.model is module:
            tr._after_model_load(module, incompatible_keys)

    def __deepcopy__(self, memo):
        return self


class WeightKeeper:
    """Keeps the KERNEL-SIDE COPIES of a model's parameters: the parameters move into one fp32 arena (same Parameter objects, same values:
    optimizers, DDP and checkpoints are unaffected), every derived copy (bf16 shadow, transposed tiles, packed fragments, remainders, conv
    repacks) is allocated and registered, and refresh_if_stale() re-derives all of them with five launches when an external optimizer has
    stepped (any parameter's version counter moved).  Gradients, optimizer state and communication are the caller's (Lightning +
    torch.optim.Adam + torch DDP: hulc2/training.py:79-82); without a keeper that loop re-derives every copy per parameter and layout through
    torch ops (~200 small launches per step).
    step_node: the keeper also owns a GRADIENT arena and registers every parameter's slice as a gradient sink that is live only inside the
    model's step node (hulc2_amd/stepnode.py: the whole forward + backward of a training step as ONE autograd node, eager or as two replayed
    hipGraphs) — the backward kernels write weight gradients straight into the arena (grouped launch, first writer overwrites), the node
    hands the arena views to autograd as the parameters' gradients."""

    def __init__(self, model: torch.nn.Module, step_node: bool = False):
        self.step_node = bool(step_node)
        fuse = self.step_node and next(p for p in model.parameters() if p.requires_grad).is_cuda
        self._install(model, plan_arena(model, fuse), grad_arena=self.step_node)
        if fuse:
            self._register_sinks(self)                     # (owner-scoped: live inside this model's step node only)

    def _install(self, model, plan, grad_arena: bool) -> None:
        """retire the model's earlier keeper, move the parameters into the arena, allocate and register every copy the plan lists (the
        device tables and the derived arenas on CUDA only), derive them"""
        self.model = model
        prev = model.__dict__.get("_hulc_arena_trainer")
        prev = prev() if prev is not None else None
        if prev is not None and prev.model is model:       # (a deep copy of a model carries the original's weak reference along)
            prev.close()                                   # its load hook would keep re-homing weights into a dead arena (and keep that arena alive)
        for mod in model.modules():                        # views installed by an earlier keeper die with its arena
            if getattr(mod, "fused_param_groups", None) is not None:
                mod._fused = None
        self.params, self.offsets, self.total = plan.params, plan.offsets, plan.total
        self.dev = dev = self.params[0].device
        cuda = dev.type == "cuda"
        bf16 = lambda n: torch.zeros(n, dtype=torch.bfloat16, device=dev)
        table = lambda a: torch.from_numpy(a).to(dev) if cuda and a is not None and len(a) else None
        self.flat_p = torch.zeros(self.total, dtype=torch.float32, device=dev)
        _ARENAS[self.flat_p.untyped_storage().data_ptr()] = self    # (hulc2_amd.optim.Adam finds the arena behind a parameter list here)
        self.flat_g = torch.zeros(self.total if grad_arena else 0, dtype=torch.float32, device=dev)
        self.grads_zeroed_at = None            # flat_g._version at which hulc2_amd.optim.Adam.zero_grad(set_to_none=False) left the arena all zeros
        self.flat_bf16 = bf16(self.total) if cuda else None
        with torch.no_grad():
            for p, off in zip(self.params, self.offsets):
                n = p.numel()
                self.flat_p[off:off + n].copy_(p.reshape(-1))
                p.data = self.flat_p[off:off + n].view(p.shape)
                if cuda and p.dim() == 2:
                    shadow.register_arena_view(p, self.flat_bf16[off:off + n].view(p.shape))
        # fused group views: parameter view for the kernels, gradient view as its sink, bf16 shadow like any 2-D weight
        self.fused = []
        for gi, (mod, g) in enumerate(plan.groups):
            off, shape = plan.group_spans[gi], tuple(g["shape"])
            n = int(np.prod(shape))
            pv, gv = self.flat_p[off:off + n].view(shape), self.flat_g[off:off + n].view(shape)
            mod._fused = dict(mod._fused or {}, **{g["attr"]: pv})
            self.fused.append((pv, gv, off, shape))
            if len(shape) == 2:
                shadow.register_arena_view(pv, self.flat_bf16[off:off + n].view(shape))
        self.tiles_t, self.frag_idx, self.lo_seg = table(plan.tiles), table(plan.frag_idx), table(plan.lo_seg)
        self.lo_frag_idx, self.conv_table = table(plan.lo_frag_idx), table(plan.conv_table)
        self.lo_ranges = plan.lo_ranges if self.lo_seg is not None else []
        self.flat_bf16_t = bf16(self.total) if self.tiles_t is not None else None
        self.frag_shadow = bf16(plan.frag_len) if self.frag_idx is not None else None
        self.flat_lo = bf16(self.total) if self.lo_seg is not None else None
        self.lo_frag = bf16(plan.lo_frag_len) if self.lo_frag_idx is not None else None
        self.conv_shadow = bf16(plan.conv_len) if self.conv_table is not None else None
        if self.tiles_t is not None:
            for t, off, (r, c) in plan.mats:
                t = self.fused[t][0] if isinstance(t, int) else t
                shadow.register_arena_view_t(t, self.flat_bf16_t[off:off + r * c].view(c, r))
        if self.lo_seg is not None:
            for p, off in plan.lo_nat:
                shadow.register_layout_view(p, "lo", self.flat_lo[off:off + p.numel()].view(p.shape))
                if p.dim() == 4:                           # conv weight: its OIHW-flat remainder is the same memory
                    shadow.register_layout_view(p, "oihw_flat_lo", self.flat_lo[off:off + p.numel()].view(p.shape[0], -1))
        for arena, views in ((self.frag_shadow, plan.frag_views), (self.lo_frag, plan.lo_frag_views), (self.conv_shadow, plan.conv_views)):
            for p, name, d0, shape in (views if arena is not None else ()):
                shadow.register_layout_view(p, name, arena[d0:d0 + p.numel()].view(shape))
        self.refresh_shadows()
        self._sink_keys = []
        self._autograd_written, self._zero_planned, self._replan_pending = set(), None, False      # (the zeroing plan of the gradient arena, below)
        # (not a bound method: copy.deepcopy(model) copies the module's hook table, and a bound method would drag the keeper — arenas and all —
        # into the copy; the copy's hook finds that the keeper belongs to another module and does nothing)
        self._load_hook = model.register_load_state_dict_post_hook(_LoadHook(self))
        model.__dict__["_hulc_arena_trainer"] = weakref.ref(self)

    def _register_sinks(self, owner) -> None:
        """every parameter's (and fused view's) slice of the gradient arena as its gradient sink (hulc2_amd/gradsink.py)"""
        for p, off in zip(self.params, self.offsets):
            self._sink_keys.append(gradsink.register(p, self.flat_g[off:off + p.numel()].view(p.shape), owner))
        for pv, gv, _, _ in self.fused:
            self._sink_keys.append(gradsink.register(pv, gv, owner))

    # ---- the gradient arena between backward passes (the step node's, or the native loop's) ---------------------------------------------------
    def _plan_partial_zero(self) -> None:
        """After a fully zeroed step: the arena slices NOT written through a gradient sink are the only ones the next steps need zeroed
        (autograd's `param.grad += g` lands there); sinks written by the backward kernels are overwritten by their first writer
        (hulc2_amd/gradsink.py).  Neighbouring must-zero slices are merged across small written ones — zeroing a slice that is overwritten
        later is harmless, one fill launch per slice is not."""
        spans = []                                                 # arena ranges of fused groups whose single sink was written
        for pv, gv, off, shape in self.fused:
            if gradsink.written(pv):
                spans.append((off, off + gv.numel()))
        inside = lambda a, b: any(lo <= a and b <= hi for lo, hi in spans)
        # ... and of those only the ones autograd really accumulates into (seen by the post-accumulate hooks during this first, fully zeroed
        # step): a parameter nobody writes (an unused module of the reference's constructor, e.g. plan_recognition.layernorm) stays zero
        need = [(off, off + p.numel()) for p, off in zip(self.params, self.offsets)
                if not (gradsink.written(p) or inside(off, off + p.numel())) and id(p) in self._autograd_written]
        self._zero_planned = {id(p) for p in self.params if id(p) in self._autograd_written}
        self._zero_ranges = merge_ranges(need, gap=1 << 18)        # gaps up to 1 MB of fp32 are cheaper to zero than another launch
        self._planned_written = gradsink.written_ids()
        self._sink_slices = {id(p): (off, off + p.numel()) for p, off in zip(self.params, self.offsets)}
        self._sink_slices.update({id(pv): (off, off + gv.numel()) for pv, gv, off, _ in self.fused})

    _zero_ranges = None

    def _zero_arena(self) -> None:
        """what a backward pass needs of the gradient arena before it starts: everything zeroed (first pass: sinks accumulate) or only the slices
        autograd accumulates into (later passes: the first sink writer of a slice overwrites it)"""
        if self._zero_ranges is None or switches.on("FULL_ZERO_GRAD"):
            self.flat_g.zero_()
            gradsink.begin_step(False)
        else:
            for a, b in self._zero_ranges:
                self.flat_g[a:b].zero_()
            gradsink.begin_step(True)

    def _settle_sinks(self) -> None:
        """bookkeeping behind a finished backward pass: the first (fully zeroed) pass makes the zeroing plan; later passes clean up after it"""
        self._settle_zeroed = []                                   # the slices this call cleared (a captured loop repeats them per replay)
        if self._zero_ranges is None and gradsink._sinks and not switches.on("FULL_ZERO_GRAD"):
            self._plan_partial_zero()                              # the backward that just finished ran on a fully zeroed arena
        elif self._zero_ranges is not None:
            # a sink the plan expects to be overwritten was not written by this backward (a branch of the model did not run): its slice
            # still holds the previous step's gradient — the true gradient is zero
            now = gradsink.written_ids()
            for k in self._planned_written - now:
                a, b = self._sink_slices[k]
                self.flat_g[a:b].zero_()
                self._settle_zeroed.append((a, b))
            # a sink written for the first time AFTER the plan was made (untouched in the planning step, so neither zeroed per step nor
            # expected to be overwritten): from now on it is "expected" — a later step that does not write it gets the clean-up above
            # instead of Adam applying the stale slice (second case)
            new = {k for k in now if k in self._sink_slices} - self._planned_written
            if new:
                self._planned_written = self._planned_written | new
            if self._replan_pending:
                # a parameter autograd accumulates into showed up after the plan: its slice was zero when this backward started (unplanned
                # slices are only ever written through sinks, and those are cleaned above), so THIS step's sum is right; the next step
                # runs on a fully zeroed arena and the plan is re-made behind it
                self._zero_ranges, self._replan_pending = None, False

    def __deepcopy__(self, memo):
        """a keeper is not copied with its model (copy.deepcopy(model) reaches it through the model's __dict__): the copy starts without one
        and builds its own on its first training step"""
        return None

    def span_ranges(self, indices) -> List[Tuple[int, int]]:
        """merged arena ranges of the parameters with these indices (into self.params)"""
        return span_ranges(self.offsets, self.total, indices)

    def refresh_if_stale(self) -> bool:
        """an external optimizer steps the parameters in place (views of the arena) and bumps their version counters; one look at them decides
        whether the derived copies are re-made (five launches for the whole model)"""
        ps = self.params
        sig = sum(p._version for p in ps)                      # (every in-place write to any parameter — optimizer, load, a test's nudge — moves it)
        if sig == getattr(self, "_fresh_sig", None):
            return False
        for p, off in zip(ps, self.offsets):                  # (an optimizer that REPLACED .data would have left the arena)
            if p.data_ptr() != self.flat_p.data_ptr() + off * 4:
                self._after_model_load(None, None)
                break
        else:
            self.refresh_shadows()
        self._fresh_sig = sig
        return True

    def _refresh_lo(self) -> None:
        """the remainders from scratch (weights written from outside; the optimizer step keeps them fresh inside its own kernel)"""
        if self.lo_seg is not None:
            kn.residual_bf16(self.flat_p, self.flat_bf16, self.flat_lo, self.lo_seg)
            if self.lo_frag_idx is not None:
                kn.gather_chunks(self.flat_lo, None, self.lo_frag, self.lo_frag_idx)

    def refresh_shadows(self) -> None:
        """Re-derive every kernel-side copy of the parameters from the fp32 arena.  The arena optimizers keep them fresh step by step
        (derive_after_step); anything else that writes the parameters (model.load_state_dict — Lightning restores weights AFTER the optimizer
        exists, hulc2/training.py:41-53,82 —, an external p.data.copy_) must be followed by this call, else the next forward/backward runs on
        the old weights.  Installed as a load_state_dict post-hook on the model."""
        if self.flat_bf16 is not None:
            kn.cast_f32_to_bf16(self.flat_p, self.flat_bf16, self.total)
            if self.tiles_t is not None:
                kn.transpose_bf16_tiles(self.flat_bf16, self.flat_bf16_t, self.tiles_t)
            if self.frag_idx is not None:
                kn.gather_chunks(self.flat_bf16, self.flat_bf16_t, self.frag_shadow, self.frag_idx)
            self._refresh_lo()
            if self.conv_table is not None:
                kn.repack_conv_weights(self.flat_p, self.conv_shadow, self.conv_table)
        shadow.bump_epoch()

    def derive_after_step(self) -> None:
        """behind ANY arena optimizer launch (it wrote the parameters, the bf16 shadow and the remainders inside lo_ranges): the other derived
        copies in two launches (were five: transposed tiles, fragment gather, residual, remainder gather, conv repack)"""
        if self.tiles_t is not None or self.conv_table is not None:
            kn.derive_copies(self.flat_bf16, self.flat_bf16_t, self.tiles_t, self.flat_p, self.conv_shadow, self.conv_table)
        if self.frag_idx is not None or self.lo_frag_idx is not None:
            kn.gather_chunks2(self.flat_bf16, self.flat_bf16_t, self.frag_shadow, self.frag_idx, self.flat_lo, self.lo_frag, self.lo_frag_idx)
        shadow.bump_epoch()

    def _after_model_load(self, module, incompatible_keys) -> None:
        for p, off in zip(self.params, self.offsets):         # a load that REPLACED .data (assign=True) would detach the arena: re-home it
            if p.data_ptr() != self.flat_p.data_ptr() + off * 4:
                with torch.no_grad():
                    self.flat_p[off:off + p.numel()].copy_(p.reshape(-1))
                    p.data = self.flat_p[off:off + p.numel()].view(p.shape)
        self.refresh_shadows()

    def close(self) -> None:
        """Detach this keeper from the model: the load_state_dict post-hook (which keeps the keeper, hence its arenas, alive through the model)
        is removed and the gradient sinks are dropped.  Parameters keep living in the arena until another keeper re-homes them."""
        h, self._load_hook = getattr(self, "_load_hook", None), None
        if h is not None:
            h.remove()
        gradsink.unregister(getattr(self, "_sink_keys", ()))       # this keeper's sinks only (another live one keeps its own)
        self._sink_keys = []

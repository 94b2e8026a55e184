"""hulc2_amd/arena.py on the host: the one interval merge against a set-of-integers model, and the arena plan of the gripper model — order,
offsets, every device table — as plain numpy data, no GPU."""
import random
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from hulc2_amd import arena  # noqa: E402
from hulc2_amd.compat import instantiate  # noqa: E402
from hulc2_amd.config import default_model_config  # noqa: E402


# ---- intervals ---------------------------------------------------------------------------------------------------------------------------
def _covered(ranges):
    return {x for a, b in ranges for x in range(a, b)}


def _runs(points):
    """maximal runs of a set of integers as (begin, end) ranges"""
    out = []
    for x in sorted(points):
        if out and out[-1][1] == x:
            out[-1][1] = x + 1
        else:
            out.append([x, x + 1])
    return [(a, b) for a, b in out]


def _random_ranges(rng):
    return [(a, a + rng.randint(1, 12)) for a in (rng.randint(0, 150) for _ in range(rng.randint(1, 14)))]


@pytest.mark.parametrize("gap", [0, 1, 3, 10])
def test_merge_ranges_covers_the_input_and_only_gaps_up_to_gap(gap):
    rng = random.Random(gap)
    for _ in range(300):
        ranges = _random_ranges(rng)
        want = _covered(ranges)
        for a, b in _runs(set(range(min(want), max(want) + 1)) - want):       # holes between covered integers
            if b - a <= gap:
                want |= set(range(a, b))
        got = arena.merge_ranges(ranges, gap)
        assert got == _runs(want), (ranges, gap, got)                          # (sorted, disjoint and maximal: the runs of the model)
    assert arena.merge_ranges([]) == [] and arena.merge_ranges([(0, 4), (4, 8), (9, 12)]) == [(0, 8), (9, 12)]


def test_close_to_keeps_at_most_limit_ranges_and_closes_the_smallest_gaps():
    rng = random.Random(7)
    for _ in range(300):
        ranges, limit = _random_ranges(rng), rng.randint(1, 5)
        merged = arena.merge_ranges(ranges)
        got = arena.close_to(ranges, limit)
        assert 1 <= len(got) <= limit and got == sorted(got) and all(b < c for (_, b), (c, _) in zip(got, got[1:])), (ranges, got)
        assert _covered(got) >= _covered(ranges)
        assert {a for a, _ in got} <= {a for a, _ in merged} and {b for _, b in got} <= {b for _, b in merged}
        gaps = sorted(c - b for (_, b), (c, _) in zip(merged, merged[1:]))
        assert len(_covered(got)) - len(_covered(ranges)) == sum(gaps[:max(len(merged) - limit, 0)]), (ranges, limit, got)
        if len(merged) <= limit:
            assert got == merged


def _legacy_skip_ranges(offsets, total, skip):
    """the span walk ArenaTrainer._skip_ranges and optim._ArenaStep._skip_ranges each wrote out before arena.span_ranges"""
    ranges = []
    for i in range(len(offsets)):
        if i not in skip:
            continue
        a, b = offsets[i], offsets[i + 1] if i + 1 < len(offsets) else total
        if ranges and ranges[-1][1] == a:
            ranges[-1][1] = b
        else:
            ranges.append([a, b])
    return [(a, b) for a, b in ranges]


# ---- the plan of the gripper model -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planned():
    model = instantiate(default_model_config(gripper_control=True))
    return model, arena.plan_arena(model, fuse=True)


def test_order_and_offsets(planned):
    model, plan = planned
    assert {id(p) for p in plan.params} == {id(p) for p in model.parameters() if p.requires_grad} and len(plan.params) == len(plan.offsets)
    assert plan.groups and plan.member
    for p, off in zip(plan.params, plan.offsets):
        if id(p) not in plan.member:
            assert off % 8 == 0
    for gi, (_, g) in enumerate(plan.groups):                                   # members back to back, in the group's order
        at = plan.group_spans[gi]
        assert at % 8 == 0
        for q in g["params"]:
            i = next(k for k, p in enumerate(plan.params) if p is q)
            assert plan.offsets[i] == at
            at += q.numel()
        assert at + g["pad"] == plan.group_spans[gi] + int(np.prod(g["shape"]))
    ends = plan.offsets[1:] + [plan.total]
    assert all(off + p.numel() <= end for p, off, end in zip(plan.params, plan.offsets, ends)) and plan.total % 8 == 0
    for gi, (_, g) in enumerate(plan.groups):                                   # the group's view, padding included, ends before the next parameter
        last = max(k for k, p in enumerate(plan.params) if any(p is q for q in g["params"]))
        assert plan.group_spans[gi] + int(np.prod(g["shape"])) <= ends[last]
    # without sinks there are no fused views: plain registration order
    flat = arena.plan_arena(model, fuse=False)
    assert not flat.groups and [id(p) for p in flat.params] == [id(p) for p in model.parameters() if p.requires_grad]
    assert all(off % 8 == 0 for off in flat.offsets)


def test_transposed_tiles_lie_inside_their_matrices(planned):
    model, plan = planned
    names = {id(p): n for n, p in model.named_parameters()}
    assert plan.tiles.dtype == np.int64 and plan.tiles.shape[1] == 5 and len(plan.tiles)
    mats = {off: shape for _, off, shape in plan.mats}
    for owner, off, (r, c) in plan.mats:
        if isinstance(owner, int):
            assert off == plan.group_spans[owner] and (r, c) == tuple(plan.groups[owner][1]["shape"])
        else:
            n = names[id(owner)]
            assert tuple(owner.shape) == (r, c) and min(r, c) >= 8 and id(owner) not in plan.member
            assert "rnn.weight_hh" not in n and "rnn.weight_ih_l1" not in n
        assert off + r * c <= plan.total
    seen = set()
    for off, r, c, i, j in plan.tiles.tolist():
        assert mats[off] == (r, c) and 0 <= 64 * i < r and 0 <= 64 * j < c and (off, i, j) not in seen
        seen.add((off, i, j))
    assert len(seen) == sum(((r + 63) // 64) * ((c + 63) // 64) for r, c in mats.values())


def test_remainder_ranges_cover_every_segment(planned):
    _, plan = planned
    assert plan.lo_seg.dtype == np.int64 and plan.lo_seg.shape[1] == 3 and len(plan.lo_seg)
    assert 1 <= len(plan.lo_ranges) <= 8 and all(a % 4 == 0 and 0 <= a < b <= plan.total for a, b in plan.lo_ranges)
    assert plan.lo_ranges == arena.merge_ranges(plan.lo_ranges)
    for src, n, dst in plan.lo_seg.tolist():
        assert src == dst and any(a <= src and src + n <= b for a, b in plan.lo_ranges)
    assert sorted(off for _, off in plan.lo_nat) == sorted(plan.lo_seg[:, 0].tolist())


@pytest.mark.parametrize("which", ["frag", "lo_frag"])
def test_fragment_indices_permute_the_chunks_of_their_own_parameter(planned, which):
    _, plan = planned
    idx, views, length = (plan.frag_idx, plan.frag_views, plan.frag_len) if which == "frag" else (plan.lo_frag_idx, plan.lo_frag_views, plan.lo_frag_len)
    off_of = {id(p): off for p, off in zip(plan.params, plan.offsets)}
    assert idx.dtype == np.int32 and views and idx.size * 4 == length == sum(n for _, _, _, n in views)
    word = idx.view(np.uint32).astype(np.int64)
    for p, name, dst, n in views:
        assert dst % 4 == 0 and n == p.numel() and n % 4 == 0
        mine = word[dst // 4:(dst + n) // 4]
        transposed = which == "frag" and name in ("ffn_p2", "ffn_p3")           # (bit 31: the chunk comes from the transposed shadow)
        assert ((mine >> 31) == int(transposed)).all(), name
        src = np.sort(mine & 0x7FFFFFFF)
        assert (src == np.arange(off_of[id(p)] // 4, (off_of[id(p)] + n) // 4)).all(), name     # every chunk of the parameter, once


def test_conv_repack_destinations_are_disjoint(planned):
    _, plan = planned
    off_of = {off: p for p, off in zip(plan.params, plan.offsets)}
    assert plan.conv_table.dtype == np.int64 and plan.conv_table.shape[1] == 7 and len(plan.conv_table) == len(plan.conv_views)
    spans = []
    for (src, dst, co, ci, kh, kw, mode), (p, name, d0, shape) in zip(plan.conv_table.tolist(), plan.conv_views):
        assert off_of[src] is p and d0 == dst and dst % 8 == 0 and co * ci * kh * kw == p.numel() == int(np.prod(shape))
        assert mode == {"oihw_flat": 0, "ohwi": 1, "ihwo": 2, "hwc": 1, "hwc_t": 3}[name]
        spans.append((dst, dst + p.numel()))
    spans.sort()
    assert all(b <= c for (_, b), (c, _) in zip(spans, spans[1:])) and spans[-1][1] <= plan.conv_len


def test_span_ranges_are_the_skip_ranges_of_before(planned):
    model, plan = planned
    # hand-written, tests/test_optim_select_cpu.py: Linear(5, 3), Linear(3, 9), Linear(9, 2) -> 15, 3, 27, 9, 18, 2 elements, padded to 8
    offsets, total = [0, 16, 24, 56, 72, 96], 104
    small = arena.plan_order(list(torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.Linear(3, 9), torch.nn.Linear(9, 2)).parameters()), [])
    assert (small[1], small[2]) == (offsets, total)
    assert arena.span_ranges(offsets, total, [2, 3, 5]) == [(24, 72), (96, 104)]                 # (ArenaTrainer(skip_params=[ps[2], ps[3], ps[5]]))
    assert arena.span_ranges(offsets, total, (i for i in range(6) if i not in {0, 1, 4})) == [(24, 72), (96, 104)]   # (the drop-in: no gradient)
    # hand-written, tests/test_optim_dropin_gpu.py: the two parameters the oracle never gives a gradient are arena neighbours -> ONE range
    names = [n for p in plan.params for n, q in model.named_parameters() if q is p]
    i = names.index("plan_recognition.layernorm.weight")
    assert names[i + 1] == "plan_recognition.layernorm.bias"
    assert arena.span_ranges(plan.offsets, plan.total, [i, i + 1]) == [(plan.offsets[i], plan.offsets[i + 2])]
    # ... and any subset, against the walk both callers used to write out
    rng = random.Random(3)
    for _ in range(50):
        skip = set(rng.sample(range(len(plan.params)), rng.randint(1, len(plan.params))))
        have = [i for i in range(len(plan.params)) if i not in skip]
        assert arena.span_ranges(plan.offsets, plan.total, (i for i in range(len(plan.params)) if i not in set(have))) == \
            _legacy_skip_ranges(plan.offsets, plan.total, skip)

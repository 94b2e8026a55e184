"""The gradient-destination protocol of hulc2_amd/gradsink.py (dest / joint / deliver) on plain CPU tensors: which tensor a backward kernel
writes, whether it accumulates, and what autograd gets back."""
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from hulc2_amd import gradsink  # noqa: E402

NAN = float("nan")


@pytest.fixture(autouse=True)
def _clean_tables():
    gradsink.clear()
    gradsink.clear_aliases()
    gradsink.begin_step(False)
    yield
    gradsink.clear()
    gradsink.clear_aliases()
    gradsink.begin_step(False)


def _params(*shapes):
    return [torch.nn.Parameter(torch.zeros(s)) for s in shapes]


def _arena(params, fill=NAN, owner=None):
    arena = torch.full((sum(p.numel() for p in params),), fill)
    off, views = 0, []
    for p in params:
        views.append(arena[off:off + p.numel()].view_as(p))
        gradsink.register(p, views[-1], owner)
        off += p.numel()
    return arena, views


def _same_memory(a, b):
    return a.data_ptr() == b.data_ptr() and a.numel() == b.numel()


def test_dest_without_a_sink_is_a_fresh_tensor_for_autograd():
    (w,) = _params((1, 6))
    like = torch.zeros(1)
    t, acc, ret = gradsink.dest(w, (3, 2), like)
    assert t.shape == (3, 2) and t.dtype == torch.float32 and t.device == like.device and acc is False and ret is t
    t, acc, ret = gradsink.dest(w, None, like)         # the parameter's own shape: (1, D) weights keep theirs
    assert t.shape == (1, 6) and acc is False and ret is t
    assert not gradsink.written(w)


def test_dest_with_a_sink_follows_the_step_mode_and_earlier_writers():
    (w,) = _params((4, 6))
    _, (view,) = _arena([w])
    like = torch.zeros(1)
    gradsink.begin_step(True)
    t, acc, ret = gradsink.dest(w, (6, 4), like)
    assert _same_memory(t, view) and t.shape == (6, 4) and acc is False and ret is None     # first writer of an overwrite step
    t, acc, ret = gradsink.dest(w, None, like)
    assert _same_memory(t, view) and t.shape == (4, 6) and acc is True and ret is None      # second writer adds
    gradsink.begin_step(False)                         # a fully zeroed step: everybody adds
    assert gradsink.dest(w, None, like)[1] is True and gradsink.dest(w, None, like)[1] is True
    gradsink.begin_step(True)
    assert gradsink.dest(w, None, like)[1] is False


def test_dest_overwrite_only_leaves_the_sink_to_the_first_writer():
    (s,) = _params(())
    _, (view,) = _arena([s])
    like = torch.zeros(1)
    gradsink.begin_step(True)
    t, acc, ret = gradsink.dest(s, None, like, overwrite_only=True)
    assert _same_memory(t, view) and acc is False and ret is None
    t, acc, ret = gradsink.dest(s, None, like, overwrite_only=True)
    assert not _same_memory(t, view) and t.shape == () and acc is False and ret is t
    gradsink.begin_step(False)
    t, acc, ret = gradsink.dest(s, None, like, overwrite_only=True)
    assert ret is t and acc is False and gradsink.written(s)         # through autograd, and still marked as written


def test_dest_resolves_an_alias_to_its_parameter():
    (w,) = _params((5,))
    _, (view,) = _arena([w])
    alias = w.detach().requires_grad_(True)
    gradsink.set_aliases([alias], [w])
    gradsink.begin_step(True)
    t, acc, ret = gradsink.dest(alias, None, alias)
    assert _same_memory(t, view) and acc is False and ret is None and gradsink.written(w)
    assert gradsink.dest(w, None, w)[1] is True        # the alias's write counts for the real parameter


def test_owner_scoped_sink_is_invisible_outside_active():
    (w,) = _params((5,))
    owner = object()
    _, (view,) = _arena([w], owner=owner)
    gradsink.begin_step(True)
    t, acc, ret = gradsink.dest(w, None, w)
    assert ret is t and not _same_memory(t, view) and not gradsink.written(w)
    assert gradsink.deliver(w, t) is t
    with gradsink.active(owner):
        t, acc, ret = gradsink.dest(w, None, w)
        assert _same_memory(t, view) and acc is False and ret is None
    assert gradsink.dest(w, None, w)[2] is not None


def test_joint_all_first_writes_overwrites_and_zeroes_nothing():
    ps = _params((4,), (4,))
    arena, views = _arena(ps)
    gradsink.begin_step(True)
    ts, acc, rets = gradsink.joint(ps, None, arena)
    assert acc is False and rets == [None, None] and all(_same_memory(t, v) for t, v in zip(ts, views))
    assert torch.isnan(arena).all()
    assert all(gradsink.written(p) for p in ps)


def test_joint_no_first_write_accumulates():
    ps = _params((4,), (2, 2))
    arena, views = _arena(ps)
    gradsink.begin_step(True)
    gradsink.joint(ps, None, arena)
    ts, acc, rets = gradsink.joint(ps, ((2, 2), None), arena)
    assert acc is True and rets == [None, None] and ts[0].shape == (2, 2) and ts[1].shape == (2, 2)
    assert torch.isnan(arena).all()                    # nothing zeroed: the first writers' values stay
    gradsink.begin_step(False)                         # a fully zeroed step: the same answer for everybody
    assert gradsink.joint(ps, None, arena)[1] is True and torch.isnan(arena).all()


def test_joint_mixed_zeroes_exactly_the_first_write_destinations():
    gamma, beta1, beta2 = ps = _params((4,), (4,), (4,))
    arena, views = _arena(ps)
    gradsink.begin_step(True)
    assert gradsink.joint((gamma, beta1), None, arena)[1] is False
    arena[:8] = 3.0                                    # what the first launch wrote
    ts, acc, rets = gradsink.joint((gamma, beta2), None, arena)
    assert acc is True and rets == [None, None]
    assert _same_memory(ts[0], views[0]) and _same_memory(ts[1], views[2])
    assert torch.equal(arena, torch.tensor([3.0] * 8 + [0.0] * 4))


def test_joint_with_one_parameter_unsunk_goes_through_autograd():
    ps = _params((4,), (4,), (2, 3))
    arena, views = _arena(ps[:2])
    gradsink.begin_step(True)
    ts, acc, rets = gradsink.joint(ps, ((2, 2), None, None), arena)
    assert acc is False and all(r is t for r, t in zip(rets, ts))
    assert [t.shape for t in ts] == [(2, 2), (4,), (2, 3)] and all(t.dtype == torch.float32 for t in ts)
    assert not any(_same_memory(t, v) for t in ts for v in views)
    assert not any(gradsink.written(p) for p in ps) and torch.isnan(arena).all()


def test_deliver_copies_then_adds_into_a_permuted_view():
    O, C, HW = 3, 4, 5
    (w,) = _params((O, C * HW))
    arena, (view,) = _arena([w])
    g = torch.arange(O * HW * C, dtype=torch.float32).view(O, HW, C)
    src = g.transpose(1, 2)                            # (O, C, HW): the parameter's column order, not contiguous
    assert not src.is_contiguous()
    want = src.reshape(O, C * HW)
    gradsink.begin_step(True)
    assert gradsink.deliver(w, src) is None and torch.equal(view, want)
    assert gradsink.deliver(w, src) is None and torch.equal(view, 2 * want)
    gradsink.begin_step(False)                         # a fully zeroed step: adds from the start
    arena.zero_()
    assert gradsink.deliver(w, src) is None and torch.equal(view, want)


def test_deliver_without_a_sink_is_a_pass_through():
    (w,) = _params((3, 20))
    src = torch.ones(3, 5, 4).transpose(1, 2)
    assert gradsink.deliver(w, src) is src and not gradsink.written(w)

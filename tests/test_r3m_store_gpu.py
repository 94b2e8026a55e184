"""VisionR3M reads the uint8 episode store in place (hulc_r3m_stage_u8): kernel, encoder, training step, captured graphs.

Everything between a stored byte and the trunk's first convolution is pointwise, and the staging kernel looks every byte up in a table the
fp32 normalisation kernel itself produced — so every comparison here is bit for bit, against the existing fp32 path run on the fp32 frames
that a torch restatement makes of the same bytes:

    restatement = store[frame_index] -> channels first, float -> replicate-pad by `pad`, integer crop at (sx, sy) -> the camera's chain

(the shift of conv1's uint8 path.  Without a shift and with the simulation chain this is oracle.frames_u8_to_input exactly —
tests/test_r3m_store_cpu.py; WITH a shift the oracle samples the crop through F.grid_sample, whose bilinear weights leave it within 6e-5 of
the integer crop, not equal to it, so the crop is restated here.)
"""
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
pytestmark = pytest.mark.gpu

from hulc2_amd import kernels as kn, switches  # noqa: E402
from hulc2_amd import synthetic as syn  # noqa: E402
from hulc2_amd.compat import instantiate  # noqa: E402
from hulc2_amd.config import real_world_model_config  # noqa: E402
from hulc2_amd.datasets import DeviceEpisodeStore  # noqa: E402
from hulc2_amd.models.perceptual_encoders import vision_r3m as VR  # noqa: E402

MEAN, STD = VR.IMAGENET_MEAN, VR.IMAGENET_STD
BF, F32 = torch.bfloat16, torch.float32


def restate(store, index, shift, pad, chain):
    """uint8 (n, H, W, 3) [+ index (N,), shift (N, 2) {sx, sy}] -> fp32 (N, 3, H, W): the frames the transforms would have delivered (CPU)"""
    fr = store if index is None else store[index.long()]
    x = fr.permute(0, 3, 1, 2).float()
    if shift is not None:
        h, w = x.shape[2:]
        xp = F.pad(x, (pad,) * 4, mode="replicate")
        x = torch.stack([xp[i, :, int(sy):int(sy) + h, int(sx):int(sx) + w] for i, (sx, sy) in enumerate(shift.tolist())])
    return VR.BYTE_CHAINS[chain](x).contiguous()


def _bytes(n, h, w, seed):
    return torch.randint(0, 256, (n, h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _stage(dev, store, index, shift, pad, chain, layout, dtype):
    """-> (the staging kernel's output on a 0xFF-filled buffer, the fp32 kernel's output on the restated frames), both on the host"""
    n, (h, w) = (store.shape[0] if index is None else index.numel()), store.shape[1:3]
    shape = (n, h + 6, kn.r3m_packed_width(w), 4) if layout == "packed" else (n, h, w, 8)
    lut = VR._byte_lut(chain, MEAN, STD, dtype, dev)
    assert lut.shape == (3, 256) and lut.dtype == dtype
    numel = shape[0] * shape[1] * shape[2] * shape[3]
    got = torch.full((numel * torch.empty(0, dtype=dtype).element_size(),), 0xFF, dtype=torch.uint8, device=dev).view(dtype).reshape(shape)
    dv = lambda t: None if t is None else t.to(dev)
    kn.r3m_stage_u8(store.to(dev), got, lut, dv(index), dv(shift), pad)
    x = restate(store, index, shift, pad, chain).to(dev)
    want = torch.full(shape, float("nan"), dtype=dtype, device=dev)
    (kn.r3m_normalize_packed if layout == "packed" else kn.r3m_normalize)(x, want, MEAN, STD)
    torch.cuda.synchronize()
    return got.cpu(), want.cpu()


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _check(got, want, layout, h, w):
    """interior = the fp32 kernel's bits; border (packed) and pad channels exactly zero (all-zero bits: + 0.0)"""
    if layout == "packed":
        inside = torch.zeros(got.shape[1:3], dtype=torch.bool)
        inside[3:3 + h, 3:3 + w] = True
        assert _same_bits(got[:, inside][..., :3], want[:, inside][..., :3])
        assert not got[:, inside][..., 3].contiguous().view(torch.int16).ne(0).any()
        assert not got[:, ~inside].contiguous().view(torch.int16).ne(0).any()
    else:
        assert _same_bits(got[..., :3], want[..., :3])
        assert not got[..., 3:].contiguous().view(torch.uint8).ne(0).any()
    assert _same_bits(got, want)              # ... and the whole buffer, zeros included, is what the fp32 kernel writes
    assert not torch.isnan(got.float()).any()


LAYOUTS = [("packed", BF), ("nhwc8", BF), ("nhwc8", F32)]
# {0, pad, 2 pad} in each coordinate independently: all nine combinations (the four corners among them), on a repeated, out-of-order index
INDEX_5 = [6, 0, 6, 3, 3]
SHIFTS_9 = [(sx, sy) for sx in (0, 4, 8) for sy in (0, 4, 8)]


@pytest.mark.parametrize("layout,dtype", LAYOUTS, ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("chain", ["real_world_r3m", "rand_shift"])
def test_stage_small_frames_every_clamp(dev, layout, dtype, chain):
    store = _bytes(7, 16, 24, 1)
    for k in range(0, 9, 5):                   # two launches of five frames cover the nine shift pairs (the last repeats the first)
        shift = torch.tensor([SHIFTS_9[(k + i) % 9] for i in range(5)], dtype=torch.int32)
        got, want = _stage(dev, store, torch.tensor(INDEX_5, dtype=torch.int32), shift, 4, chain, layout, dtype)
        _check(got, want, layout, 16, 24)


@pytest.mark.parametrize("layout,dtype", LAYOUTS, ids=lambda v: str(v).replace("torch.", ""))
def test_stage_without_index_and_shift(dev, layout, dtype):
    store = _bytes(7, 16, 24, 2)
    got, want = _stage(dev, store, None, None, 4, "real_world_r3m", layout, dtype)
    _check(got, want, layout, 16, 24)
    # a shift of (pad + 1, pad) moves the picture one column: the kernel does look at its shift argument
    one = torch.tensor([[5, 4]] * 7, dtype=torch.int32)
    moved, want1 = _stage(dev, store, None, one, 4, "real_world_r3m", layout, dtype)
    _check(moved, want1, layout, 16, 24)
    assert not _same_bits(moved, got)
    centred, _ = _stage(dev, store, None, torch.tensor([[4, 4]] * 7, dtype=torch.int32), 4, "real_world_r3m", layout, dtype)
    assert _same_bits(centred, got)


@pytest.mark.parametrize("layout,dtype", LAYOUTS, ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("hw", [(150, 200), (200, 200)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_stage_shipped_sizes(dev, hw, layout, dtype):
    """the two shipped static-camera sizes; the index names the LAST store frame, whose last window ends at the store's last byte"""
    store = _bytes(4, *hw, 3)
    index = torch.tensor([3, 0, 3], dtype=torch.int32)
    shift = torch.tensor([[20, 20], [0, 7], [13, 20]], dtype=torch.int32)
    got, want = _stage(dev, store, index, shift, 10, "rand_shift", layout, dtype)
    _check(got, want, layout, *hw)


# ---- (b) the encoder ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net(dev):
    m = VR.VisionR3M(dev, 64).to(dev)
    syn.fill_state_dict_(m.state_dict(), 11)
    return m


def test_width_must_be_a_multiple_of_four(dev, net):
    store = _bytes(2, 16, 22, 4).to(dev)
    y = torch.empty(2, 16, 22, 8, dtype=BF, device=dev)
    with pytest.raises(ValueError, match="22"):
        kn.r3m_stage_u8(store, y, VR._byte_lut("real_world_r3m", MEAN, STD, BF, dev))
    with pytest.raises(ValueError, match="22"):
        net(store)


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("hw,chain,pad", [((150, 200), "real_world_r3m", 4), ((200, 200), "rand_shift", 10)], ids=["150x200-rw", "200x200-sim"])
def test_encoder_on_bytes_equals_encoder_on_fp32_frames(dev, net, mode, hw, chain, pad):
    store = _bytes(9, *hw, 5)
    index = torch.tensor([8, 2, 2, 0, 7, 8], dtype=torch.int32)
    shift = torch.randint(0, 2 * pad + 1, (6, 2), generator=torch.Generator().manual_seed(6), dtype=torch.int32)
    shift[0], shift[1] = torch.tensor([2 * pad, 0]), torch.tensor([0, 2 * pad])
    x = restate(store, index, shift, pad, chain)
    kn.set_compute(mode)
    try:
        net.input_chain = chain
        with torch.no_grad():
            want = net(x.to(dev))
            got = net(store.to(dev), shift.to(dev), pad, index.to(dev))
            gathered = net(store[index.long()].to(dev), shift.to(dev), pad)          # uint8 frames without an index
            two = net([store.to(dev), store.to(dev)], [shift.to(dev), None], pad, [index.to(dev), index.to(dev)])
            plain = net(restate(store, index, None, pad, chain).to(dev))
        with pytest.raises(TypeError):
            net(x.to(dev), shift.to(dev), pad)                                        # fp32 frames arrive shifted
    finally:
        net.__dict__.pop("input_chain", None)
        kn.set_compute("bf16")
    assert got.shape == (6, 64) and torch.isfinite(got).all()
    assert torch.equal(got, want) and torch.equal(gathered, want)
    assert torch.equal(two[:6], want) and torch.equal(two[6:], plain) and not torch.equal(plain, want)


# ---- (c) the step, (d) the captured step --------------------------------------------------------------------------------------------------
def _stores(dev, S=4):
    """one synthetic real-world split of 40 frames (150 x 200 static, 84 x 84 gripper) as two datasets: play windows and language windows"""
    g = torch.Generator().manual_seed(17)
    n, ids = 40, [(0, 17), (18, 39)]
    rgb = {"rgb_static": torch.randint(0, 256, (n, 150, 200, 3), generator=g, dtype=torch.uint8),
           "rgb_gripper": torch.randint(0, 256, (n, 84, 84, 3), generator=g, dtype=torch.uint8)}
    act, obs = torch.rand(n, 7, generator=g) * 2 - 1, torch.randn(n, 15, generator=g)
    kw = dict(min_window_size=2, max_window_size=S, device=dev, aug_pad={"rgb_static": 0})
    vis = DeviceEpisodeStore(rgb, act, obs, ids, seed=3, **kw)
    lang = DeviceEpisodeStore(vis.rgb, act, obs, ids, seed=4, lang_emb=torch.randn(5, 384, generator=g) * 0.05,
                              lang_lookup=torch.randint(0, 5, (len(vis),), generator=g).tolist(), **kw)
    return {"vis": vis, "lang": lang}


def _rw_model(dev, seed):
    kn.set_compute("bf16")
    m = instantiate(real_world_model_config(dropout_p=0.0)).to(dev)
    syn.fill_state_dict_(m.state_dict(), seed)
    m.train()
    return m


CHECKED = ["perceptual_encoder.rgb_static_encoder.fc1.weight", "perceptual_encoder.rgb_static_encoder.fc1.bias",
           "perceptual_encoder.rgb_static_encoder.fc2.weight", "perceptual_encoder.rgb_static_encoder.fc2.bias",
           "perceptual_encoder.rgb_gripper_encoder.conv_model.0.weight"]


def test_training_step_from_the_store_equals_fp32_static_frames(dev):
    m = _rw_model(dev, 21)
    stores = _stores(dev)
    idxs = {"vis": [1, len(stores["vis"]) - 1], "lang": [5, 20]}            # (the last start of the last episode: a padded window)
    by_index, materialised = {}, {}
    for mod, st in stores.items():
        db = st.batch(idxs[mod])
        db = {k: (dict(v) if isinstance(v, dict) else v) for k, v in db.items()}
        assert "rgb_static_shift" not in db["rgb_obs"] and "rgb_gripper_shift" in db["rgb_obs"]
        by_index[mod] = db
        fd = dict(db)
        fd["rgb_obs"] = dict(db["rgb_obs"])
        ix = fd["rgb_obs"].pop("rgb_static_index").long()
        fd["rgb_obs"]["rgb_static"] = st.rgb["rgb_static"][ix].permute(0, 1, 4, 2, 3).float().contiguous()      # (B, S, 3, H, W) in [0, 255]
        materialised[mod] = fd
    assert (by_index["vis"]["window_sizes"] < 4).any()
    outs = []
    for bt in (materialised, by_index):
        for p in m.parameters():
            p.grad = None
        kn.reset_step_state(dev)
        loss = m.training_step(bt, 0)
        loss.backward()
        torch.cuda.synchronize()
        outs.append((loss.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}))
    kn.check_faults(dev)
    assert torch.isfinite(outs[0][0]) and torch.equal(outs[0][0], outs[1][0])
    assert outs[0][1].keys() == outs[1][1].keys()
    for k in CHECKED:
        assert float(outs[0][1][k].abs().max()) > 0 and torch.equal(outs[0][1][k], outs[1][1][k]), k


DRAWS = [{"vis": [1, 30], "lang": [5, 20]}, {"vis": [0, 14], "lang": [33, 2]}, {"vis": [9, 35], "lang": [11, 12]},
         {"vis": [22, 3], "lang": [0, 35]}, {"vis": [16, 17], "lang": [7, 27]}]


def _in_child(case: str) -> None:
    """run `_case_<case>(dev)` of this file in a fresh interpreter; its output is shown, a non-zero exit status fails the test.  The cases
    that capture graphs run this way, as in tests/test_kl_beta_gpu.py: the suite's later step-node tests then see the number of earlier
    captures they saw without this file (hipGraphLaunch on this runtime depends on a process's capture history: NOTES "Round 6")."""
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), case], capture_output=True, text=True, timeout=600)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, f"child `{case}` exited with {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"


def _store_loop(dev, graphs: bool):
    kn.reset_step_state(dev)
    m = _rw_model(dev, 23)
    stores = _stores(dev)
    losses = []
    with switches.scope(HULC_NO_STEP_GRAPH=None if graphs else "1"):      # (read when the model's step node is made)
        for i, d in enumerate(DRAWS):
            for p in m.parameters():
                p.grad = None
            loss = m.training_step({mod: st.batch(d[mod]) for mod, st in stores.items()}, i)
            loss.backward()
            losses.append(float(loss.detach()))
    torch.cuda.synchronize()
    kn.check_faults(dev)
    return losses, m.__dict__["_hulc_step_node"]


def _case_step_node(dev):
    want, eager = _store_loop(dev, graphs=False)
    assert eager.captures == 0 and eager.eager_steps == 5
    got, node = _store_loop(dev, graphs=True)
    print(f"[step node] eager losses {want}\n[step node] graph losses {got}")
    assert node.disabled is None, node.disabled
    assert node.captures == 1 and node.replays == 3 and node.eager_steps == 2
    assert node.input_copies == 0 and not node.slot_idx
    assert len(set(want)) == 5, want                  # five different batches
    assert got == want, (got, want)


def test_captured_step_follows_the_store(dev):
    """five draws of store windows: the step node runs two eagerly, captures on the third and replays it, the fourth and the fifth — the
    captured launches read the store through the index / shift buffers that batch() refreshed in place: no frame slot, no input copy —
    and the five losses are those of the eager node (HULC_NO_STEP_GRAPH=1) on the same draws"""
    _in_child("step_node")


def _case_native_loop(dev):
    from hulc2_amd.trainer import ArenaTrainer

    def run(graph):
        kn.reset_step_state(dev)
        tr = ArenaTrainer(_rw_model(dev, 29), overlap=False)
        stores, batch = _stores(dev), {}

        def draw(d):
            for mod, st in stores.items():
                batch[mod] = st.batch(d[mod])

        draw(DRAWS[0])
        if graph:
            tr.capture(batch)
        else:
            for i in range(2):                                     # capture()'s two warm-up steps
                tr.step(batch, i)
        losses = []
        for d in DRAWS[1:]:
            draw(d)
            losses.append(float(tr.replay() if graph else tr.step(batch, 0)))
        torch.cuda.synchronize()
        kn.check_faults(dev)
        return losses, tr.flat_p.clone()

    want, p_want = run(False)
    got, p_got = run(True)
    print(f"[native loop] eager losses {want}\n[native loop] replay losses {got}")
    assert len(set(want)) == 4 and all(x == x for x in want), want
    assert got == want, (got, want)
    assert torch.equal(p_got, p_want)


def test_arena_trainer_graphs_follow_the_store(dev):
    """the native loop: ArenaTrainer.capture on store windows, then replays after batch() drew other windows into the same buffers — losses and
    all parameters bit-equal to a twin trainer taking the same steps eagerly"""
    _in_child("native_loop")


if __name__ == "__main__":
    assert torch.cuda.is_available()
    globals()["_case_" + sys.argv[1]](torch.device("cuda:0"))

"""Host mirror of the counter-based RNG (test infrastructure only, like the rest of oracle/).

hulc2_amd/csrc/hulc_common.h draws every dropout mask and plan sample from a pure function of (seed, index): no mask tensor exists on the
device, so a reference that replays the device's masks has to recompute them.  This file restates that function in vectorised numpy uint64
and maps the transformer trunk's mask sites (hulc2_amd/functional.py transformer_encoder_layer / TxlBlockFn, AddPosFn) to element indices.

A kernel's seed is its site id XOR the device RNG word (kernels.step_state(dev)[0]); the site ids of the trunk are derived from the call's
site `s`: the position add draws from `s`, layer l from s' = s + 100 (l + 1): attention probabilities s' + 11, the out_proj residual branch
s' + 12, the feed-forward hidden activation s' + 13, the linear2 residual branch s' + 15.
"""
from typing import Dict, List

import numpy as np

U64 = np.uint64
MASK64 = (1 << 64) - 1


def _u64(v) -> np.uint64:
    return U64(int(v) & MASK64)


def rand64(seed, idx) -> np.ndarray:
    """hulc_rand64: two rounds of a 64-bit multiply-xorshift of idx * golden + seed (wrapping arithmetic)"""
    idx = np.asarray(idx, dtype=U64)
    with np.errstate(over="ignore"):
        z = idx * U64(0x9E3779B97F4A7C15) + _u64(seed)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def uniform01(seed, idx) -> np.ndarray:
    """hulc_uniform01: the top 24 bits of the draw's upper word, in [0, 1) as float32"""
    r32 = rand64(seed, idx) >> U64(32)
    return (r32 >> U64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def keep_scale(p: float) -> np.float32:
    """1.0f / (1.0f - p) in fp32"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def dropout_scale(seed, idx, p: float) -> np.ndarray:
    """dropout_scale: element idx keeps (scale 1 / (1 - p), else 0) when 16-bit lane idx & 3 of draw idx >> 2 reaches (uint32)(p * 65536.0f)"""
    idx = np.asarray(idx, dtype=U64)
    thr = np.uint64(int(np.float32(p) * np.float32(65536.0)))
    u = (rand64(seed, idx >> U64(2)) >> (U64(16) * (idx & U64(3)))) & U64(0xFFFF)
    return np.where(u >= thr, keep_scale(p), np.float32(0.0)).astype(np.float32)


def keep_probability(p: float) -> float:
    """the exact keep probability of dropout_scale: 1 - floor(p * 2^16) / 2^16"""
    return 1.0 - int(np.float32(p) * np.float32(65536.0)) / 65536.0


# ------------------------------------------------------------------------------------------------
# the transformer trunk's sites
# ------------------------------------------------------------------------------------------------
POS, ATTN, OUT, FFN, LIN2 = "pos", "attn", "out", "ffn", "lin2"
LAYER_SITES = {ATTN: 11, OUT: 12, FFN: 13, LIN2: 15}
# the call sites (hulc2_amd/models/plan_encoders/plan_recognition_net.py): the batched call over all modalities' rows (modality-major), and
# the per-modality calls of Hulc2.lmp_train and of the per-modality training step
TRUNK_SITE = 0x5EED0001
MODALITY_SITES = {"vis": 0x5EED1001, "lang": 0x5EED2001}


def layer_site(site: int, layer: int, what: str) -> int:
    return site + 100 * (layer + 1) + LAYER_SITES[what]


def trunk_masks(p: float, site: int, word: int, B: int, S: int, E: int = 128, H: int = 8, FF: int = 2048, L: int = 2,
                row0: int = 0) -> Dict[str, object]:
    """the keep-scales (float32, 0 or 1 / (1 - p)) of every mask of one trunk call over rows row0 .. row0 + B - 1 of its batch (a slice of a
    call over more rows: the modalities of the batched call), drawn with the device RNG word `word`:
      pos (B, S, E)          dropout(emb + pos)              index (b S + t) E + e
      layers[l] = dict(
        attn (B, H, S, S)    attention probabilities         index ((b H + h) S + i) S + j
        out  (B, S, E)       out_proj residual branch        index tok E + e      (tok = b S + t)
        ffn  (B, S, FF)      feed-forward hidden activation  index tok FF + j
        lin2 (B, S, E))      linear2 residual branch         index tok E + e"""
    b = np.arange(row0, row0 + B, dtype=np.uint64)

    def flat(*shape):                                      # row-major flat indices of a (B, *shape) block starting at row row0
        n = int(np.prod(shape))
        return b.reshape(-1, *([1] * len(shape))) * U64(n) + np.arange(n, dtype=np.uint64).reshape(shape)

    def draw(s, idx):
        return dropout_scale(int(s) ^ (int(word) & MASK64), idx, p)

    out = {POS: draw(site, flat(S, E)), "layers": []}
    for layer in range(L):
        out["layers"].append({ATTN: draw(layer_site(site, layer, ATTN), flat(H, S, S)), OUT: draw(layer_site(site, layer, OUT), flat(S, E)),
                              FFN: draw(layer_site(site, layer, FFN), flat(S, FF)), LIN2: draw(layer_site(site, layer, LIN2), flat(S, E))})
    return out


def trunk_site_ids(site: int, L: int = 2) -> List[int]:
    """every sub-site a trunk call with site `site` draws from"""
    return [site] + [layer_site(site, layer, w) for layer in range(L) for w in (ATTN, OUT, FFN, LIN2)]


def sample_classes(logits: np.ndarray, seed: int, word: int, g0: int = 0, margin: float = 1e-5):
    """plan_sample_kernel without injected indices: group g (32 classes; g0 + the row-major group number of `logits` in the launch) takes
    the first class whose inclusive CDF exceeds hulc_uniform01(seed ^ word, g) — here on a float64 CDF.  -> (class (G,), trusted (G,)):
    groups whose uniform lies within margin x total of a CDF boundary are not trusted (the kernel sums its fp32 CDF in another order)."""
    lg = np.asarray(logits, dtype=np.float64).reshape(-1, 32)
    e = np.exp(lg - lg.max(axis=1, keepdims=True))
    cdf = np.cumsum(e, axis=1) / e.sum(axis=1, keepdims=True)
    u = uniform01(int(seed) ^ (int(word) & MASK64), np.arange(g0, g0 + lg.shape[0], dtype=np.uint64)).astype(np.float64)
    cls = np.minimum((cdf > u[:, None]).argmax(axis=1), 31)
    cls = np.where((cdf > u[:, None]).any(axis=1), cls, 31)
    trusted = np.abs(cdf - u[:, None]).min(axis=1) > margin
    return cls, trusted

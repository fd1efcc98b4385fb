"""numpy restatement of the packed policy / value net (include/skyjo_vec.h: "The packed layout") and of torch.optim.Adam's
documented rule in float64 - the reference of tests/test_gpu_mlp_update.py.  Written from the two documents; it shares no code with the
library.  Also the inputs those tests use (weight set B, the hand-made gradients), so that the CPU tests can look at them first.

The blob, pieces back to back in skyjo_vec_mlp_export's order (a fragment = 8 bf16 = 16 bytes; value j of lane l, hh = l >> 5):
    w1 [8 u][2 s][64 l][8 j]   bf16(S * W1[32 u + (l & 31)][k]),  k = 16 s + 8 hh + j;  k = 31 carries b1, k in [obs_dim, 31) is 0
    w2 [8 u][16 ks][64 l][8 j] hi(S * W2[32 u + (l & 31)][acc_k(ks, hh, j)])
    w3 [16 ks][64 l][8 j]      hi(W3[l & 31][acc_k]), rows >= out_dim: hi(0)
    b2 float32 [256],  b3 float32 [64 l][16 r] (row (r & 3) + 8 (r >> 2) + 4 hh)
    w1l, w2l, w3l              "fp32" only: lo(v) = bf16(v - float(bf16(v)))
"""
import numpy as np

SCALE = np.float32(2.8853900817779268)  # 2 / ln 2, rounded to float32
H, IN, OUT = 256, 32, 32
F32 = np.float32


def bf16(x):
    """float32 -> bf16 bits (uint16): round to nearest even on the bit pattern."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFFFFFF) >> 16).astype(np.uint16)


def bf16_value(h):
    return (np.asarray(h, dtype=np.uint16).astype(np.uint32) << 16).view(F32)


def bf16_lo(x):
    x = np.ascontiguousarray(x, dtype=F32)
    return bf16(x - bf16_value(bf16(x)))  # one float32 subtraction


def acc_k(ks, hh, j):
    return 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * hh + (j & 3)


def _hi(v, precision):
    return bf16(v) if precision == "fp32" else bf16(F32(-2.0) * v)


def _row_sum(bias, rows, precision):
    """bias + (bf16 mode) the row's bf16-rounded weights, in double, ascending k."""
    b = bias.astype(np.float64)
    if precision == "bf16":
        r = bf16_value(bf16(rows)).astype(np.float64)
        for k in range(H):
            b = b + r[:, k]
    return b.astype(F32)


def tables(w1, b1, w2, b2, w3, b3):
    """The three layers as the packed net sees them, float32: V1 [256][32] (scaled, bias in column 31), V2 [256][256] (scaled),
    V3 [32][256] (rows >= out_dim zero)."""
    w1, b1, w2, b2, w3, b3 = (np.ascontiguousarray(a, dtype=F32) for a in (w1, b1, w2, b2, w3, b3))
    obs_dim, out_dim = w1.shape[1], w3.shape[0]
    assert w1.shape == (H, obs_dim) and 1 <= obs_dim <= IN - 1 and w2.shape == (H, H) and w3.shape == (out_dim, H) and 1 <= out_dim <= OUT
    v1 = np.zeros((H, IN), dtype=F32)
    v1[:, :obs_dim] = w1
    v1[:, IN - 1] = b1
    v3 = np.zeros((OUT, H), dtype=F32)
    v3[:out_dim] = w3
    return SCALE * v1, SCALE * w2, v3


def pieces(w1, b1, w2, b2, w3, b3, precision="fp32"):
    """name -> array of the piece, in the blob's order."""
    assert precision in ("fp32", "bf16")
    v1, v2, v3 = tables(w1, b1, w2, b2, w3, b3)
    out_dim = np.shape(w3)[0]
    u, s, l, j = np.indices((8, 2, 64, 8))
    i1 = (32 * u + (l & 31), 16 * s + 8 * (l >> 5) + j)
    u, ks, l, j = np.indices((8, 16, 64, 8))
    i2 = (32 * u + (l & 31), acc_k(ks, l >> 5, j))
    ks, l, j = np.indices((16, 64, 8))
    i3 = (l & 31, acc_k(ks, l >> 5, j))
    b3row = np.zeros((OUT,), dtype=F32)
    b3row[:out_dim] = _row_sum(np.asarray(b3, dtype=F32), v3[:out_dim], precision)
    l, r = np.indices((64, 16))
    p = {"w1": bf16(v1[i1]), "w2": _hi(v2[i2], precision), "w3": _hi(v3[i3], precision),
         "b2": _row_sum(SCALE * np.asarray(b2, dtype=F32), v2, precision), "b3": b3row[(r & 3) + 8 * (r >> 2) + 4 * (l >> 5)]}
    if precision == "fp32":
        p.update(w1l=bf16_lo(v1[i1]), w2l=bf16_lo(v2[i2]), w3l=bf16_lo(v3[i3]))
    return p


def pack(w1, b1, w2, b2, w3, b3, precision="fp32"):
    """The bytes skyjo_vec_mlp_export gives for a net of these weights: uint8 [168 960] ("bf16") or [332 800] ("fp32")."""
    return np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in pieces(w1, b1, w2, b2, w3, b3, precision).values()])


def unpack(blob, precision="fp32"):
    """The inverse, from the blob alone and by the inverse index maps (where does weight (m, k) lie?), not by pack's tables:
    {"w1": [256][32], "w2": [256][256], "w3": [32][256]} uint16 high halves, the same with an "l" suffix for the low halves ("fp32"),
    "b2" float32 [256], "b3" float32 [32] (checked to be the same in all the lanes that hold a row)."""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    sizes = [("w1", 8 * 2 * 64 * 8, np.uint16), ("w2", 8 * 16 * 64 * 8, np.uint16), ("w3", 16 * 64 * 8, np.uint16), ("b2", H, F32), ("b3", 64 * 16, F32)]
    if precision == "fp32":
        sizes += [("w1l", 8 * 2 * 64 * 8, np.uint16), ("w2l", 8 * 16 * 64 * 8, np.uint16), ("w3l", 16 * 64 * 8, np.uint16)]
    raw, at = {}, 0
    for name, n, dt in sizes:
        nb = n * np.dtype(dt).itemsize
        raw[name] = blob[at:at + nb].view(dt)
        at += nb
    assert at == blob.size, (at, blob.size)
    out = {"b2": raw["b2"].copy()}
    m, k = np.indices((H, IN))
    at1 = (((m >> 5) * 2 + (k >> 4)) * 64 + (m & 31) + 32 * ((k >> 3) & 1)) * 8 + (k & 7)
    m, k = np.indices((H, H))
    ks, lane_hi, j = 2 * (k >> 5) + ((k >> 4) & 1), (k >> 2) & 1, 4 * ((k >> 3) & 1) + (k & 3)
    at2 = (((m >> 5) * 16 + ks) * 64 + (m & 31) + 32 * lane_hi) * 8 + j
    m3, k = np.indices((OUT, H))
    ks, lane_hi, j = 2 * (k >> 5) + ((k >> 4) & 1), (k >> 2) & 1, 4 * ((k >> 3) & 1) + (k & 3)
    at3 = (ks * 64 + m3 + 32 * lane_hi) * 8 + j
    for suffix in ("", "l") if precision == "fp32" else ("",):
        out["w1" + suffix], out["w2" + suffix], out["w3" + suffix] = raw["w1" + suffix][at1], raw["w2" + suffix][at2], raw["w3" + suffix][at3]
    for a in (at1, at2, at3):
        assert np.unique(a).size == a.size  # every position is hit once: (m, k) -> position is a bijection
    assert at1.size == raw["w1"].size and at2.size == raw["w2"].size and at3.size == raw["w3"].size
    b3 = raw["b3"].reshape(64, 16)
    rows = np.zeros((OUT,), dtype=F32)
    for lane in range(64):
        for r in range(16):
            row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
            if lane & 31 == 0:
                rows[row] = b3[lane, r]
            assert b3[lane, r].view(np.uint32) == rows[row].view(np.uint32)
    out["b3"] = rows
    return out


def adam_ref(p, g, m, v, lr, betas, eps, t):
    """torch.optim.Adam's documented rule (no amsgrad, no weight decay) in float64, step t counting from 1: (p, m, v)."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    b1, b2 = float(betas[0]), float(betas[1])
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    p = p - (float(lr) / (1.0 - b1 ** t)) * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + float(eps))
    return p, m, v


# ---- the inputs of tests/test_gpu_mlp_update.py ----
SHAPES = ((31, 26), (31, 1), (17, 26), (1, 32))


def _scaled_hits(want_low, bit16, count, rng):
    """float32 w whose S * w (one float32 multiply) has the low 16 bits `want_low` and bit 16 equal to `bit16`: found by search."""
    hits = []
    while len(hits) < count:
        target = ((int(rng.integers(0x3000, 0x4400)) << 16) & 0x7FFE0000) | (bit16 << 16) | want_low | (int(rng.integers(0, 2)) << 31)
        w = np.array([target], dtype=np.uint32).view(F32) / SCALE
        for cand in (w, np.nextafter(w, F32(np.inf)), np.nextafter(w, F32(-np.inf))):
            bits = int((SCALE * cand).view(np.uint32)[0])
            if bits & 0xFFFF == want_low and (bits >> 16) & 1 == bit16:
                hits.append(cand[0])
                break
    return np.array(hits[:count], dtype=F32)


def weights_b(obs_dim, out_dim, seed=1234):
    """Weight set B (w1, b1, w2, b2, w3, b3): both signs everywhere, magnitudes 1e-30 .. 1e4, and in every tensor exact bf16 ties
    of the stored value in both directions of the even rule (bit 16 clear: down, set: up), values whose low half is zero, +0, -0
    and a float32 subnormal."""
    rng = np.random.default_rng(seed)
    shapes = ((H, obs_dim), (H,), (H, H), (H,), (out_dim, H), (out_dim,))
    out = []
    for i, shape in enumerate(shapes):
        n = int(np.prod(shape))
        x = (10.0 ** rng.uniform(-30, 4, n) * rng.choice([-1.0, 1.0], n)).astype(F32)
        scaled = i < 4  # layers 1 and 2 and their biases are stored times S; layer 3 and b3 as they are
        if scaled:
            special = [_scaled_hits(0x8000, 0, 3, rng), _scaled_hits(0x8000, 1, 3, rng), _scaled_hits(0, 0, 2, rng), _scaled_hits(0, 1, 2, rng)]
        else:
            mk = lambda bits: np.array(bits, dtype=np.uint32).view(F32)
            special = [mk([0x3F808000, 0xBE428000, 0x40A48000]), mk([0x3F818000, 0xBE438000, 0x40A58000]), mk([0x3F000000, 0xBFA00000]),
                       mk([0x3F810000, 0xC0490000])]
        special = np.concatenate(special + [np.array([0.0, -0.0, 1e-40, -3e-42, 1e-30, -1e4, 1e4, 1.1754944e-38], dtype=F32)])
        # spread over the tensor, first and last element included
        pos = list(dict.fromkeys([0, n - 1] + rng.permutation(n)[:special.size].tolist()))[:special.size]
        x[pos] = special[:len(pos)]
        out.append(x.reshape(shape))
    return out


ADAM_HYPER = dict(lr=float(F32(3e-4)), betas=(float(F32(0.9)), float(F32(0.999))), eps=float(F32(1e-8)))  # float32 values: the ABI's type
ADAM_STEPS = 3
ADAM_ZERO_TENSOR = 3  # (index into w1, b1, w2, b2, w3, b3 of one branch) this tensor's gradient is all zero in every step


def adam_grads(shapes, step, seed=77):
    """Hand-made float32 gradients of one branch for step 1, 2, 3: magnitudes 1e-12 .. 1e3, both signs, tensor ADAM_ZERO_TENSOR all
    zero, a few exact zeros elsewhere."""
    rng = np.random.default_rng(seed + 1000 * step)
    out = []
    for i, shape in enumerate(shapes):
        n = int(np.prod(shape))
        g = (10.0 ** rng.uniform(-12, 3, n) * rng.choice([-1.0, 1.0], n)).astype(F32)
        g[rng.choice(n, size=max(1, n // 50), replace=False)] = 0.0
        if i == ADAM_ZERO_TENSOR:
            g[:] = 0.0
        out.append(g.reshape(shape))
    return out

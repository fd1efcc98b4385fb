"""numpy restatement of the packed net's layout for any 1 <= obs_dim <= 163 (include/skyjo_vec.h: "The packed layout"): the
reference of tests/test_gpu_net_wide.py.  Layer 1 takes KS = obs_dim // 16 + 1 k-steps of 16 columns (two below 16 inputs: the narrow
nets' blob as it always was), K = 16 KS: column k < obs_dim is
feature k, columns obs_dim .. K - 2 are zero, column K - 1 carries b1 (scaled like the weights); the w1 piece (and "fp32": w1l) is
[8 u][KS s][64 l][8 j] in the natural k order k = 16 s + 8 hh + j.  Everything else - layers 2 and 3, the biases, the order of the
pieces - is tests/mlp_pack_ref.py's, whose functions are used for it; for obs_dim <= 31 the bytes are that module's.  Not collected: a helper.
"""
import numpy as np

from tests import mlp_pack_ref as pk

H, OUT, F32, SCALE = pk.H, pk.OUT, pk.F32, pk.SCALE
MAX_OBS = 163
WIDE_OBS = (32, 43, 47, 48, 67, 163)
WIDE_SHAPES = tuple((d, o) for d in WIDE_OBS for o in (26, 1))


def ksteps(obs_dim):
    assert 1 <= obs_dim <= MAX_OBS
    return max(2, obs_dim // 16 + 1)


def columns(obs_dim):
    return 16 * ksteps(obs_dim)


def table1(w1, b1):
    """Layer 1 as the packed net sees it: float32 [256][K], scaled, the bias in column K - 1."""
    w1, b1 = np.ascontiguousarray(w1, dtype=F32), np.ascontiguousarray(b1, dtype=F32)
    obs_dim = w1.shape[1]
    assert w1.shape == (H, obs_dim) and b1.shape == (H,)
    K = columns(obs_dim)
    v1 = np.zeros((H, K), dtype=F32)
    v1[:, :obs_dim] = w1
    v1[:, K - 1] = b1
    return SCALE * v1


def _narrow_stand_in(params):
    """The same net with a one-input layer 1: what tests/mlp_pack_ref.py packs of layers 2 and 3 does not depend on layer 1."""
    return (np.zeros((H, 1), dtype=F32), np.zeros((H,), dtype=F32)) + tuple(params[2:])


def pieces(w1, b1, w2, b2, w3, b3, precision="fp32"):
    """name -> array of the piece, in the blob's order."""
    params = (w1, b1, w2, b2, w3, b3)
    v1 = table1(w1, b1)
    KS = v1.shape[1] // 16
    u, s, l, j = np.indices((8, KS, 64, 8))
    i1 = (32 * u + (l & 31), 16 * s + 8 * (l >> 5) + j)
    rest = pk.pieces(*_narrow_stand_in(params), precision=precision)
    p = {"w1": pk.bf16(v1[i1])}
    p.update((k, rest[k]) for k in ("w2", "w3", "b2", "b3"))
    if precision == "fp32":
        p["w1l"] = pk.bf16_lo(v1[i1])
        p.update((k, rest[k]) for k in ("w2l", "w3l"))
    return p


def pack(w1, b1, w2, b2, w3, b3, precision="fp32"):
    """The bytes skyjo_vec_mlp_export gives for a net of these weights."""
    return np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in pieces(w1, b1, w2, b2, w3, b3, precision).values()])


def packed_bytes(obs_dim, precision):
    w1 = 8 * ksteps(obs_dim) * 64 * 16
    rest = (8 * 16 + 16) * 64 * 16
    return (w1 + rest) * (2 if precision == "fp32" else 1) + H * 4 + 64 * 16 * 4


def unpack(blob, obs_dim, precision="fp32"):
    """The inverse, by the inverse index map of layer 1 (where does weight (m, k) lie?): as mlp_pack_ref.unpack, with "w1" (and "w1l")
    uint16 [256][K]."""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    KS = ksteps(obs_dim)
    n1 = 8 * KS * 64 * 16
    n23 = (8 * 16 + 16) * 64 * 16
    nb = H * 4 + 64 * 16 * 4
    assert blob.size == packed_bytes(obs_dim, precision), (blob.size, packed_bytes(obs_dim, precision))
    narrow1 = np.zeros((8 * 2 * 64 * 16,), dtype=np.uint8)
    # layers 2 / 3 and the biases through mlp_pack_ref.unpack, with a narrow layer-1 piece of zeros in front
    parts = [narrow1, blob[n1:n1 + n23 + nb]]
    if precision == "fp32":
        parts += [narrow1, blob[n1 + n23 + nb + n1:]]
    out = pk.unpack(np.concatenate(parts), precision)
    m, k = np.indices((H, 16 * KS))
    at1 = (((m >> 5) * KS + (k >> 4)) * 64 + (m & 31) + 32 * ((k >> 3) & 1)) * 8 + (k & 7)
    assert np.unique(at1).size == at1.size == n1 // 2
    out["w1"] = blob[:n1].view(np.uint16)[at1]
    if precision == "fp32":
        lo = n1 + n23 + nb
        out["w1l"] = blob[lo:lo + n1].view(np.uint16)[at1]
    return out


def default_init(obs_dim, out_dim, seed):
    """torch's default initialisation of one branch under a seed: (w1, b1, w2, b2, w3, b3) float32."""
    import torch
    from torch import nn

    torch.manual_seed(seed)
    seq = nn.Sequential(nn.Linear(obs_dim, H), nn.Tanh(), nn.Linear(H, H), nn.Tanh(), nn.Linear(H, out_dim))
    return [p.detach().numpy().copy() for p in seq.parameters()]

"""tests/mlp_pack_wide_ref.py is what it claims, without a GPU: for the narrow shapes its bytes are tests/mlp_pack_ref.py's, and for wide
ones unpack(pack(p)) returns the rounded parameters with the bias in column K - 1 and zeros between."""
import numpy as np
import pytest

from tests import mlp_pack_ref as pk, mlp_pack_wide_ref as wide

PRECISIONS = ("fp32", "bf16")


def test_ksteps_at_the_edges():
    assert [wide.ksteps(d) for d in (1, 15, 16, 31, 32, 43, 47, 48, 67, 163)] == [2, 2, 2, 2, 3, 3, 3, 4, 5, 11]
    assert wide.columns(47) == 48 and wide.columns(48) == 64        # 47: the bias lands in the last free column; 48: a k-step more
    with pytest.raises(AssertionError):
        wide.ksteps(0)
    with pytest.raises(AssertionError):
        wide.ksteps(164)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", pk.SHAPES)
def test_narrow_shapes_give_the_narrow_bytes(shape, precision):
    for params in (pk.weights_b(*shape), wide.default_init(shape[0], shape[1], 0)):
        assert np.array_equal(wide.pack(*params, precision=precision), pk.pack(*params, precision=precision))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", wide.WIDE_SHAPES)
def test_unpack_of_pack_is_the_rounded_parameters(shape, precision):
    obs_dim, out_dim = shape
    params = pk.weights_b(obs_dim, out_dim)
    blob = wide.pack(*params, precision=precision)
    assert blob.size == wide.packed_bytes(obs_dim, precision)
    u = wide.unpack(blob, obs_dim, precision)
    K = wide.columns(obs_dim)
    assert u["w1"].shape == (256, K) and K - 1 >= obs_dim
    w1, b1 = params[0], params[1]
    assert np.array_equal(u["w1"][:, :obs_dim], pk.bf16(pk.SCALE * w1))
    assert not u["w1"][:, obs_dim:K - 1].any()
    assert np.array_equal(u["w1"][:, K - 1], pk.bf16(pk.SCALE * b1))
    if precision == "fp32":
        assert np.array_equal(u["w1l"][:, :obs_dim], pk.bf16_lo(pk.SCALE * w1))
        assert not u["w1l"][:, obs_dim:K - 1].any()
        assert np.array_equal(u["w1l"][:, K - 1], pk.bf16_lo(pk.SCALE * b1))
    # layers 2 and 3: what the narrow restatement says of the same parameters
    narrow = pk.unpack(pk.pack(np.zeros((256, 1), np.float32), np.zeros(256, np.float32), *params[2:], precision=precision), precision)
    for name in ("w2", "w3", "b2", "b3") + (("w2l", "w3l") if precision == "fp32" else ()):
        assert np.array_equal(np.asarray(u[name]).view(np.uint8), np.asarray(narrow[name]).view(np.uint8)), name


@pytest.mark.parametrize("precision", PRECISIONS)
def test_round_trip_and_size_at_every_wide_obs_dim(precision):
    """Every obs_dim 32 .. 163 (the GPU sweep compares FusedNet.export() with pack() at each): the size, the round trip of layer 1 with
    the bias in column K - 1 and zeros between, and the size grows by one k-step's fragments exactly where obs_dim passes a multiple of 16."""
    step = 8 * 64 * 16 * (2 if precision == "fp32" else 1)
    for obs_dim in range(32, wide.MAX_OBS + 1):
        out_dim = 26 if obs_dim % 2 else 1
        params = pk.weights_b(obs_dim, out_dim)
        blob = wide.pack(*params, precision=precision)
        K = wide.columns(obs_dim)
        assert K == 16 * (obs_dim // 16 + 1) and blob.size == wide.packed_bytes(obs_dim, precision)
        assert wide.packed_bytes(obs_dim, precision) - wide.packed_bytes(obs_dim - 1, precision) == (step if obs_dim % 16 == 0 else 0)
        u = wide.unpack(blob, obs_dim, precision)
        for name, rounded in (("w1", pk.bf16),) + ((("w1l", pk.bf16_lo),) if precision == "fp32" else ()):
            assert u[name].shape == (256, K), (obs_dim, name)
            assert np.array_equal(u[name][:, :obs_dim], rounded(pk.SCALE * params[0])), (obs_dim, name)
            assert not u[name][:, obs_dim:K - 1].any() and np.array_equal(u[name][:, K - 1], rounded(pk.SCALE * params[1])), (obs_dim, name)
        narrow = pk.unpack(pk.pack(np.zeros((256, 1), np.float32), np.zeros(256, np.float32), *params[2:], precision=precision), precision)
        for name in ("w2", "w3", "b2", "b3") + (("w2l", "w3l") if precision == "fp32" else ()):
            assert np.array_equal(np.asarray(u[name]).view(np.uint8), np.asarray(narrow[name]).view(np.uint8)), (obs_dim, name)


def test_pieces_start_where_the_narrow_blob_has_them_at_two_ksteps():
    """obs_dim <= 31 is KS = 2: every piece's size - and so its offset - is the narrow blob's."""
    params = pk.weights_b(31, 26)
    for precision in PRECISIONS:
        a, b = wide.pieces(*params, precision=precision), pk.pieces(*params, precision=precision)
        assert list(a) == list(b) and all(a[k].nbytes == b[k].nbytes for k in a)

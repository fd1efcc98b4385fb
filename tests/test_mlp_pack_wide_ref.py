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


def test_pieces_start_where_the_narrow_blob_has_them_at_two_ksteps():
    """obs_dim <= 31 is KS = 2: every piece's size - and so its offset - is the narrow blob's."""
    params = pk.weights_b(31, 26)
    for precision in PRECISIONS:
        a, b = wide.pieces(*params, precision=precision), pk.pieces(*params, precision=precision)
        assert list(a) == list(b) and all(a[k].nbytes == b[k].nbytes for k in a)

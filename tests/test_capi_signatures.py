"""include/skyjo_vec.h against skyjo_rl_amd/_lib.py, type by type, as the C++ compiler reads the header (tests/abi_probe.py).

tests/test_capi_symbols.py holds the NAMES of the signature table and four sizeofs; every GPU test calls through that table, at
sizes where an int32 in place of an int64_t, a float in place of a double or a missing trailing pointer goes unnoticed.  Here
every prototype, every structure field and every mirrored #define is compared, and the comparison itself is shown to reject
three wrong tables and one wrong structure.
"""
import ctypes as C
import subprocess

import pytest

from skyjo_rl_amd import _lib

from tests import abi_probe

CLASSES = {label: getattr(_lib, label) for label in abi_probe.STRUCTS}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    consts = dict(abi_probe.CONSTANTS)
    consts["PROF_KERNELS"] = abi_probe.PROF_KERNELS_DEFINE
    src = abi_probe.generate(_lib.SIGNATURES, abi_probe.struct_spec(CLASSES), consts)
    try:
        return abi_probe.run(src, tmp_path_factory.mktemp("abi_probe"))
    except subprocess.CalledProcessError as e:
        pytest.fail(f"the probe does not compile against include/skyjo_vec.h:\n{e.stderr}")


def test_every_prototype_matches_the_header(probe):
    assert sorted(probe.functions) == sorted(_lib.SIGNATURES)
    bad = abi_probe.signature_mismatches(probe, _lib.SIGNATURES)
    assert not bad, "\n".join(bad)


def test_row_counts_are_64_bit_in_the_header(probe):
    """The promise the GPU tests of tests/test_gpu_big_rows.py lean on: the calls that take a row count take it as 8 bytes."""
    for name, pos in (("skyjo_vec_unpack", 2), ("skyjo_vec_unpack_tiles", 2), ("skyjo_vec_sample_actions_layout", 4),
                      ("skyjo_vec_mlp_forward_layout", 4), ("skyjo_vec_mlp_act_value_layout", 5), ("skyjo_vec_rollout_select", 2),
                      ("skyjo_vec_rollout_gather", 5), ("skyjo_vec_rollout_gather_logits", 1), ("skyjo_vec_rollout_gather_logits", 3),
                      ("skyjo_vec_ppo_loss", 8), ("skyjo_vec_ppo_loss_kl", 9), ("skyjo_vec_episode_stats", 2)):
        args = probe.functions[name].split("(")[1].rstrip(")").split(",")
        assert args[pos] == "i8", (name, pos, args[pos])


def test_every_structure_field_matches_the_header(probe):
    bad = abi_probe.struct_mismatches(probe, CLASSES)
    assert not bad, "\n".join(bad)


def test_game_state_dtype_matches_the_header(probe):
    dt = _lib.GAME_STATE_DTYPE
    assert dt.itemsize == probe.sizes["GameState"]
    assert list(dt.names) == [f[0] for f in _lib.GameState._fields_]
    bad = [f"{n}: header {probe.fields[('GameState', n)]}, dtype {(dt.fields[n][1], dt.fields[n][0].itemsize)}"
           for n in dt.names if probe.fields[("GameState", n)] != (dt.fields[n][1], dt.fields[n][0].itemsize)]
    assert not bad, "\n".join(bad)


def test_every_mirrored_constant_matches_the_header(probe):
    mirrored = abi_probe.mirrored_names(_lib)
    missing = [n for n in mirrored if n not in abi_probe.CONSTANTS]
    assert not missing, f"_lib.py mirrors {missing}; tests/abi_probe.py CONSTANTS does not list them"
    assert sorted(abi_probe.CONSTANTS) == mirrored
    bad = [f"{n}: header {probe.constants[n]}, _lib {getattr(_lib, n)}" for n in mirrored if probe.constants[n] != getattr(_lib, n)]
    assert not bad, "\n".join(bad)
    assert probe.constants["PROF_KERNELS"] == len(_lib.PROF_KERNELS)


def test_integration_md_config_block_is_the_binding():
    assert abi_probe.integration_config_fields() == _lib.Config._fields_


# --- the comparison must be able to fail ---------------------------------------------------------------------------------

def _wrong_tables():
    I32, I64, VP = C.c_int32, C.c_int64, C.c_void_p
    res, args = _lib.SIGNATURES["skyjo_vec_rollout_select"]
    assert args[2] is I64
    narrowed = (res, args[:2] + [I32] + args[3:])
    res, args = _lib.SIGNATURES["skyjo_vec_ppo_loss"]
    assert args[-1] is VP
    dropped = (res, args[:-1])
    res, args = _lib.SIGNATURES["skyjo_vec_mlp_adam_step"]
    assert args[5] is C.c_float
    widened = (res, args[:5] + [C.c_double] + args[6:])
    return {"skyjo_vec_rollout_select": narrowed, "skyjo_vec_ppo_loss": dropped, "skyjo_vec_mlp_adam_step": widened}


@pytest.mark.parametrize("name", sorted(_wrong_tables()))
def test_a_wrong_table_is_rejected(probe, name):
    table = dict(_lib.SIGNATURES)
    table[name] = _wrong_tables()[name]
    bad = abi_probe.signature_mismatches(probe, table)
    assert len(bad) == 1 and bad[0].startswith(name + ":"), bad


def test_a_structure_with_two_fields_swapped_is_rejected(probe):
    fields = list(_lib.PPOUpdateArgs._fields_)
    i, j = [f[0] for f in fields].index("first_step"), [f[0] for f in fields].index("layout")
    assert C.sizeof(fields[i][1]) != C.sizeof(fields[j][1])
    fields[i], fields[j] = fields[j], fields[i]

    class Swapped(C.Structure):
        _fields_ = fields

    bad = abi_probe.struct_mismatches(probe, {"PPOUpdateArgs": Swapped})
    assert any(b.startswith("PPOUpdateArgs.first_step:") for b in bad) and any(b.startswith("PPOUpdateArgs.layout:") for b in bad), bad
    # same-sized neighbours too: offsets alone give them away
    fields = list(_lib.Config._fields_)
    fields[1], fields[2] = fields[2], fields[1]

    class Swapped2(C.Structure):
        _fields_ = fields

    bad = abi_probe.struct_mismatches(probe, {"Config": Swapped2})
    assert sorted(b.split(":")[0] for b in bad) == ["Config.num_envs", "Config.num_players"], bad


def test_a_field_the_header_lacks_does_not_compile(tmp_path):
    src = abi_probe.generate([], {"Info": ("skyjo_vec_info", ["num_envs", "no_such_field"])})
    with pytest.raises(subprocess.CalledProcessError):
        abi_probe.run(src, tmp_path)

"""CPU tests of the two reward types the device episode loop gained (reward_conditioned, distance_to_logs): the numpy
restatement of the counter-based weight generator (csrc/episode.hip), the host-side resolution of the preset / fixed
weights against the reference's formulas (gpudrive/env/env_torch.py:247-401, bounds gpudrive/env/config.py:103-113),
the argument checks, and the exports of the built library.  `draw_weights_np` is the statement the GPU tests compare
the device draws with, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from gpudrive_lab_amd import _capi
from gpudrive_lab_amd import episode as E

f32 = np.float32
_M1, _M2, _GOLD = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB), np.uint64(0x9E3779B97F4A7C15)


def _mix64(z):
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
    return z ^ (z >> np.uint64(31))


def draw_weights_np(seed, world, draw, A, lb=E.DEFAULT_LB, ub=E.DEFAULT_UB):
    """Draw `draw` of world `world` in the "random" condition mode: [A, 3] float32.  key = mix(seed ^ mix(world << 32 |
    draw)); x = mix(key + (3 slot + component + 1) * golden); u = (x >> 40) * 2^-24; w = lb + u * f32(ub - lb)."""
    key = _mix64(np.array([seed], np.uint64) ^ _mix64(np.array([(world << 32) | draw], np.uint64)))
    ctr = np.arange(1, 3 * A + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = _mix64(key + ctr * _GOLD)
    u = (x >> np.uint64(40)).astype(np.uint32).astype(f32) * f32(2.0 ** -24)
    lo, hi = np.asarray(lb, f32), np.asarray(ub, f32)
    rng = (hi - lo).astype(f32)
    return (np.tile(lo, A) + u * np.tile(rng, A)).astype(f32).reshape(A, 3)


def test_generator_in_bounds():
    lb, ub = (-1.0, 1.0, -1.0), (0.0, 2.0, 0.0)
    for w in range(4):
        for k in range(3):
            x = draw_weights_np(7, w, k, 128, lb, ub)
            assert x.dtype == f32 and x.shape == (128, 3)
            assert (x >= np.asarray(lb, f32)).all() and (x < np.asarray(ub, f32)).all(), (w, k)
    # over many draws the distribution is the reference's U[lb, ub) per component
    x = np.concatenate([draw_weights_np(1, w, 0, 128) for w in range(64)])
    mean = x.mean(axis=0)
    assert np.allclose(mean, (np.asarray(E.DEFAULT_LB) + np.asarray(E.DEFAULT_UB)) / 2, atol=0.02), mean
    assert np.allclose(x.std(axis=0), 1 / np.sqrt(12), atol=0.01)


def test_generator_is_a_function_of_its_key_and_counter():
    a = draw_weights_np(3, 5, 2, 64)
    assert np.array_equal(a.view(np.uint32), draw_weights_np(3, 5, 2, 64).view(np.uint32))
    # slot j's values do not depend on how many slots are drawn (counter, not a sequence)
    assert np.array_equal(a.view(np.uint32), draw_weights_np(3, 5, 2, 128)[:64].view(np.uint32))
    for other in (draw_weights_np(3, 6, 2, 64), draw_weights_np(3, 5, 3, 64), draw_weights_np(4, 5, 2, 64)):
        assert (other != a).mean() > 0.99


def test_presets_and_fixed_resolve_to_the_reference_values():
    lb, ub = E.DEFAULT_LB, E.DEFAULT_UB
    want = {
        "cautious": (-1.0 * 0.9, 2.0 * 0.7, -1.0 * 0.9),
        "aggressive": (-1.0 * 0.5, 2.0 * 0.9, -1.0 * 0.6),
        "balanced": ((-1.0 + 0.0) / 2, (1.0 + 2.0) / 2, (-1.0 + 0.0) / 2),
        "risk_taker": (-1.0 * 0.3, 2.0, -1.0 * 0.4),
    }
    assert set(E.PRESETS) == set(want)
    for name, vals in want.items():
        mode, w = E.resolve_condition("preset", name, lb, ub)
        assert mode == _capi.CONDITION_PRESET and w.dtype == f32
        assert np.array_equal(w.view(np.uint32), np.asarray(vals, f32).view(np.uint32)), name
    import torch
    for given in (torch.tensor([-0.75, 1.0, -0.5]), np.array([0.1, 0.2, 0.3]), [0.1, 0.2, 0.3]):
        mode, w = E.resolve_condition("fixed", given)
        assert mode == _capi.CONDITION_FIXED
        assert np.array_equal(w, np.asarray(given, f32))
    mode, w = E.resolve_condition("random")
    assert mode == _capi.CONDITION_RANDOM and not w.any()


@pytest.mark.parametrize("mode,agent_type", [
    ("uniform", None), ("preset", "reckless"), ("preset", None), ("fixed", None), ("fixed", [1.0, 2.0]),
    ("fixed", np.zeros((1, 3))), ("fixed", "cautious")])
def test_bad_condition_is_a_value_error(mode, agent_type):
    with pytest.raises(ValueError):
        E.resolve_condition(mode, agent_type)


def test_reward_types_and_struct_layout():
    assert E.REWARD_TYPES["reward_conditioned"] == 2 and E.REWARD_TYPES["distance_to_logs"] == 3
    assert "distance_to_vdb_trajs" not in E.REWARD_TYPES
    # gd_episode_config: 5 x 4 bytes, log_distance_weight, condition_mode, weights[3], lb[3], ub[3], then the 64-bit seed
    assert _capi.GdEpisodeConfig.seed.offset == 64 and C.sizeof(_capi.GdEpisodeConfig) == 72
    assert _capi.GdEpisodeBuffers.reward_weights.offset == 13 * 8 and C.sizeof(_capi.GdEpisodeBuffers) == 15 * 8
    # existing callers build the structs from the first fields only: the new ones are zero
    c = _capi.GdEpisodeConfig(-0.5, 1.0, -0.5, 0, 1)
    assert c.log_distance_weight == 0.0 and c.condition_mode == 0 and c.seed == 0 and list(c.weights) == [0, 0, 0]


def test_library_exports_the_new_entry_points():
    L = C.CDLL(_capi.lib_path())
    for name in ("gd_pack_observations_conditioned", "gd_episode_draw_weights"):
        assert hasattr(L, name), name

"""CPU suite of the dropout mask rule (csrc/dropout_rule.hpp): the generator's known answers, the feature map, the drop
statistics, and that the host program, a plain Python statement and `DropoutRule`'s host side agree."""
import numpy as np
import pytest

from gpudrive_lab_amd import _capi
from tests import dropout_reference as DREF

# counter, key -> output: the Random123 known answers of philox4x32_10
KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
         ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
          (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


def test_philox_known_answers_on_the_host_program_and_in_python():
    for counter, key, want in KNOWN:
        assert DREF.philox4x32_10(counter, key) == want
        assert DREF.host_philox(counter, key) == want
    rng = np.random.default_rng(3)
    for _ in range(20):
        w = [int(v) for v in rng.integers(0, 2 ** 32, 6)]
        assert DREF.host_philox(w[:4], w[4:]) == DREF.philox4x32_10(w[:4], w[4:])


def test_the_feature_map_is_a_bijection_and_follows_the_accumulator_layout():
    m = DREF.host_map()
    assert m.shape == (128, 2)
    for width, blocks in ((64, 8), (128, 16)):
        pairs = {(int(b), int(f)) for b, f in m[:width]}
        assert pairs == {(b, f) for b in range(blocks) for f in range(8)}
    # register r = 8 m + k of tile t in lane half h holds feature 32 t + (r & 3) + 8 (r >> 2) + 4 h: block ((2 t + m) << 1 | h), field k
    for t in range(4):
        for h in range(2):
            for r in range(16):
                f = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h
                assert tuple(m[f]) == ((((t << 1) | (r >> 3)) << 1) | h, r & 7)


@pytest.mark.parametrize("p", [0.01, 0.5])
def test_drop_counts_lie_within_four_binomial_standard_deviations(p):
    from gpudrive_lab_amd.dropout import check_rule_args
    _, _, T, scale = check_rule_args(p, 42)
    assert T == int(np.floor(p * 65536)) and scale == float(np.float32(1) / (np.float32(1) - np.float32(p)))
    keep = DREF.host_mask(42, 5, T, 2, 8, 200, 64)   # 102,400 elements
    n = keep.size
    q = T / 65536.0
    drops, sigma = int(n - keep.sum()), np.sqrt(n * q * (1 - q))
    print("p = %g: T = %d, %d drops of %d, expected %.0f, sigma %.1f" % (p, T, drops, n, n * q, sigma))
    assert n >= 100000 and abs(drops - n * q) <= 4 * sigma
    # per feature column too: no field of the 8 is stuck
    per = (~keep).reshape(-1, 64).sum(0)
    rows = n // 64
    assert (np.abs(per - rows * q) <= 5 * np.sqrt(rows * q * (1 - q)) + 1).all()


def test_the_mask_is_a_function_of_every_coordinate_and_python_agrees():
    T = 32768
    base = DREF.host_mask(7, 3, T, 1, 3, 63, 64)
    assert np.array_equal(base, DREF.host_mask(7, 3, T, 1, 3, 63, 64))
    assert not np.array_equal(base, DREF.host_mask(7, 4, T, 1, 3, 63, 64)), "call"
    assert not np.array_equal(base, DREF.host_mask(7, 3 + 2 ** 32, T, 1, 3, 63, 64)), "the call's high word"
    assert not np.array_equal(base, DREF.host_mask(8, 3, T, 1, 3, 63, 64)), "seed"
    assert not np.array_equal(base, DREF.host_mask(7 + 2 ** 32, 3, T, 1, 3, 63, 64)), "the seed's high word"
    assert not np.array_equal(base, DREF.host_mask(7, 3, T, 2, 3, 63, 64)), "site"
    assert not np.array_equal(base[0], base[1]) and not np.array_equal(base[1], base[2]), "row"
    assert len({base[0, e].tobytes() for e in range(63)}) == 63, "entity"
    assert len({base[0, :, f].tobytes() for f in range(64)}) == 64, "feature"
    shared = DREF.host_mask(7, 3, T, 3, 2, 1, 128)
    assert not np.array_equal(shared[0, 0, :64], shared[0, 0, 64:])
    rng = np.random.default_rng(0)
    for _ in range(200):
        r, e, f = int(rng.integers(0, 3)), int(rng.integers(0, 63)), int(rng.integers(0, 64))
        assert DREF.kept_python(7, 3, r, 1, e, f, T) == base[r, e, f]
    # a lower threshold only ever keeps more
    assert (DREF.host_mask(7, 3, 655, 1, 3, 63, 64) >= base).all()


def test_the_rule_refuses_on_the_host(monkeypatch):
    from gpudrive_lab_amd.dropout import DropoutRule
    monkeypatch.setattr(_capi, "lib", lambda: pytest.fail("the library is not needed for a refusal"))
    for p, seed in ((0.0, 1), (1.0, 1), (-0.1, 1), (2.0 ** -17, 1), (float("nan"), 1), (True, 1), ("0.1", 1), (None, 1),
                    (0.1, -1), (0.1, 2 ** 64), (0.1, 1.5), (0.1, True), (0.1, None), (1.0 - 2.0 ** -30, 1)):
        with pytest.raises(ValueError):
            DropoutRule(p, seed)
    with pytest.raises(ValueError):
        DropoutRule(0.1, 1, device="cpu")
    with pytest.raises(ValueError):
        DropoutRule(0.1, 1, device="no such device")

"""CPU tests of the warm-up of the device auto-reset (gd_episode_set_warmup, EpisodeTracker / DeviceLearnerEnv init_steps):
what can be checked without a device."""
import os
import re
import subprocess

import pytest

from gpudrive_lab_amd import _capi
from gpudrive_lab_amd.episode import EpisodeTracker
from gpudrive_lab_amd.learner import DeviceLearnerEnv

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpudrive_amd.h")


def test_the_setter_is_exported_and_bound():
    so = _capi.lib_path()
    if not os.path.exists(so):
        _capi.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert "gd_episode_set_warmup" in names
    assert "gd_episode_set_warmup" in _capi.SYMBOLS
    assert len(_capi.lib().gd_episode_set_warmup.argtypes) == 3


def test_scope_constants_match_the_header():
    text = open(HEADER).read()
    m = re.search(r"enum\s*\{\s*GD_WARMUP_RESET_WORLDS\s*=\s*(\d+)\s*,\s*GD_WARMUP_ALL_WORLDS\s*=\s*(\d+)\s*\}", text)
    assert m, "GD_WARMUP_* constants missing from the header"
    assert (int(m.group(1)), int(m.group(2))) == (_capi.WARMUP_RESET_WORLDS, _capi.WARMUP_ALL_WORLDS)
    assert "int gd_episode_set_warmup(gd_sim *sim, int32_t init_steps, int32_t scope);" in text
    assert _capi.STAT_WARMED_WORLDS == 46 and _capi.INIT_STEPS_MAX == 90


def _set_warmup(k, scope):
    """The engine checks the arguments before the simulator: with a null simulator an accepted pair fails on the simulator
    only (the message names it), a refused one on the argument."""
    L = _capi.lib()
    rc = L.gd_episode_set_warmup(None, k, scope)
    return rc, L.gd_last_error().decode()


@pytest.mark.parametrize("k,scope,what", [(-1, 0, "init_steps"), (91, 0, "init_steps"), (91, 1, "init_steps"),
                                          (1 << 30, 1, "init_steps"), (11, 2, "scope"), (11, -1, "scope")])
def test_setter_refuses_bad_arguments(k, scope, what):
    rc, msg = _set_warmup(k, scope)
    assert rc == _capi.GD_ERR_INVALID
    assert what in msg and "null sim" not in msg, msg


@pytest.mark.parametrize("k,scope", [(0, 0), (0, 1), (90, 0), (90, 1), (11, 0)])
def test_setter_accepts_the_range(k, scope):
    rc, msg = _set_warmup(k, scope)
    assert rc == _capi.GD_ERR_INVALID and "null sim" in msg, msg


class _NoSim:
    """Stands in for a SimManager where the checks must fire before the simulator is touched."""

    def __getattr__(self, name):
        raise AssertionError("the simulator was touched (%s) before the arguments were checked" % name)


BAD = [dict(init_steps=-1), dict(init_steps=91), dict(init_steps=1.5), dict(init_steps="11"), dict(init_steps=True),
       dict(init_steps=11, warmup="some_worlds"), dict(init_steps=0, warmup=None)]


@pytest.mark.parametrize("kw", BAD, ids=[repr(k) for k in BAD])
def test_episode_tracker_checks_before_the_device(kw):
    with pytest.raises(ValueError):
        EpisodeTracker(_NoSim(), **kw)


@pytest.mark.parametrize("kw", BAD, ids=[repr(k) for k in BAD])
def test_device_learner_env_checks_before_the_device(kw):
    with pytest.raises(ValueError):
        DeviceLearnerEnv(_NoSim(), **kw)

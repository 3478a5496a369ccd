"""MI355X-native GPUDrive step engine: host-side package.

`gpudrive_lab_amd.madrona_gpudrive_impl` mirrors the reference's `madrona_gpudrive` nanobind
module (reference src/bindings.cpp) on top of the C ABI in include/gpudrive_amd.h; the top-level
`madrona_gpudrive` package re-exports it so existing `gpudrive.env` code imports it unchanged.
"""
from ._capi import build, lib_path  # noqa: F401


def __getattr__(name):
    # torch is imported only when the module that needs it is asked for
    if name in ("TrainableBCPolicy", "TrainableBCPolicyDim"):
        from . import bc_train
        return getattr(bc_train, name)
    if name in ("DeviceBC", "DeviceBCDim"):
        from . import bc_opt
        return getattr(bc_opt, name)
    if name in ("ClosedLoopBC", "ClosedLoopEpisode"):
        from . import bc_rollout
        return getattr(bc_rollout, name)
    if name in ("ClosedLoopPPO", "PolicyEpisode"):
        from . import ppo_rollout
        return getattr(ppo_rollout, name)
    if name in ("ClosedLoopMultiPPO", "MultiPolicyEpisode"):
        from . import multi_policy_rollout
        return getattr(multi_policy_rollout, name)
    if name == "DeviceLinearProbe":
        from .lp_probe import DeviceLinearProbe
        return DeviceLinearProbe
    if name == "ProbeReadout":
        from .bc_readout import ProbeReadout
        return ProbeReadout
    raise AttributeError("module %r has no attribute %r" % (__name__, name))

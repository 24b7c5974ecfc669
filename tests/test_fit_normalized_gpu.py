"""GPU suite: the ``normalize`` keyword of ensemble.fit_weights / fit_joint / fit_joint_resampled with ``where="device"`` (the members normalised by
mms_normalize_members, then the unchanged sweep) against ``where="host"`` (ensemble.normalize_members, then the host sweep): the same tuple, the values
bit for bit; and ``normalize="none"`` against the call without the keyword."""
import functools

import numpy as np
import pytest
import torch

import joint_tables
from normalize_tables import MODES
from kddcup_2020_multimodalitiesrecall_2nd_place_amd import ensemble

pytestmark = pytest.mark.gpu

ROWS = [12] * 16


@functools.lru_cache(maxsize=None)
def _case():
    q, p, mem, key = joint_tables.table(4, ROWS)
    return q, p, mem, key, joint_tables.weights(), joint_tables.filters()


@functools.lru_cache(maxsize=None)
def _host_joint(mode):
    q, p, mem, key, grid, filters = _case()
    with np.errstate(invalid="ignore"):
        return ensemble.fit_joint(q, p, mem, key, grid, filters, where="host", normalize=mode)


def _same_joint(got, want):
    assert repr(got[:4]) == repr(want[:4])
    assert got[4].dtype == np.float64 and got[4].shape == want[4].shape and got[4].tobytes() == want[4].tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_fit_joint_device_equals_host(mode):
    q, p, mem, key, grid, filters = _case()
    info = {}
    got = ensemble.fit_joint(q, p, torch.from_numpy(mem).cuda(), key, grid, filters, where="device", normalize=mode, info=info)
    assert info == {"path": "device", "flags": 0, "normalize": mode}
    _same_joint(got, _host_joint(mode))
    assert got[4].tobytes() != _host_joint("none")[4].tobytes()              # the scale reaches the sweep


@pytest.mark.parametrize("mode", MODES)
def test_fit_weights_device_equals_host(mode):
    q, p, mem, key, grid, _ = _case()
    want = ensemble.fit_weights(q, p, mem, key, grid, where="host", normalize=mode)
    info = {}
    got = ensemble.fit_weights(q, p, mem, key, grid, where="device", normalize=mode, info=info)
    assert info == {"path": "device", "flags": 0, "normalize": mode}
    assert repr(got[:3]) == repr(want[:3]) and got[3].tobytes() == want[3].tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_fit_joint_resampled_device_equals_host(mode):
    q, p, mem, key, grid, filters = _case()
    kw = dict(scheme="kfold", folds=5, repeats=1, seed=3, normalize=mode)
    info = {}
    got = ensemble.fit_joint_resampled(q, p, mem, key, grid, filters, where="device", info=info, **kw)
    assert info["path"] == "device" and info["normalize"] == mode
    with np.errstate(invalid="ignore"):
        want = ensemble.fit_joint_resampled(q, p, mem, key, grid, filters, where="host", **kw)
    _same_joint(got["whole"], want["whole"])
    _same_joint(got["whole"], _host_joint(mode))
    assert got["winners"].shape == (5, 2) and np.array_equal(got["winners"], want["winners"])
    for name in ("fit_values", "eval_values", "probe_fit", "probe_eval"):
        assert got[name].tobytes() == want[name].tobytes(), name
    assert repr((got["heldout"], got["optimism"], got["agreement"])) == repr((want["heldout"], want["optimism"], want["agreement"]))


def test_none_is_the_call_without_the_keyword():
    q, p, mem, key, grid, filters = _case()
    dmem = torch.from_numpy(mem).cuda()
    info = {}
    _same_joint(ensemble.fit_joint(q, p, dmem, key, grid, filters, normalize="none", info=info), ensemble.fit_joint(q, p, dmem, key, grid, filters))
    assert info == {"path": "device", "flags": 0}                            # today's dict
    a, b = ensemble.fit_weights(q, p, dmem, key, grid, normalize="none"), ensemble.fit_weights(q, p, dmem, key, grid)
    assert repr(a[:3]) == repr(b[:3]) and a[3].tobytes() == b[3].tobytes()
    a, b = (ensemble.fit_joint_resampled(q, p, dmem, key, grid, filters, folds=5, repeats=1, **kw) for kw in (dict(normalize="none"), {}))
    _same_joint(a["whole"], b["whole"])
    assert a["eval_values"].tobytes() == b["eval_values"].tobytes() and np.array_equal(a["winners"], b["winners"])

"""The hidden record of the perception model, { 1e12, 1e12, type, 0 }, is neutral: the premise of "slots stay in
place".  On the CPU oracle, over 64 generated scenes at 8 and at 64 obstacles, a 128 x 128 grid and 8 ticks: a slice whose last entry is
the record gives the PlanOut, SceneState and GridOut of the slice with obs_n - 1, byte for byte, while removing the entry does change
them; and a hidden entry in the MIDDLE of the slice gives those of the slice with the entry deleted."""
import os

import numpy as np
import pytest

import dmpp_amd as dm
import oracle_binding
import perception_model as pcm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TICKS = 8


def _oracle():
    return oracle_binding.Oracle(os.path.join(ROOT, "oracle", "liboracle.so"))


def _run(orc, cfg, sc):
    st = sc["state"].copy()
    plan, gout, _ = orc.plan_tick_batch(cfg, sc, st, n_ticks=TICKS)
    return plan, st, gout


def _copy(sc):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sc.items()}


def _hide(sc, s, j):
    e = sc["obs_pool"][int(sc["scene_in"]["obs_off"][s]) + j]
    e["x"], e["y"], e["radius"] = pcm.HIDDEN_XY, pcm.HIDDEN_XY, 0.0          # (the type stays the truth's)


def _same(a, b, what):
    for x, y, name in zip(a, b, ("PlanOut", "SceneState", "GridOut")):
        assert x.tobytes() == y.tobytes(), f"{what}: {name} differs in " + ", ".join(f for f in x.dtype.names if x[f].tobytes() != y[f].tobytes())


@pytest.mark.parametrize("n_obs", [8, 64])
def test_hidden_last_entry_is_the_shorter_slice(n_obs):
    cfg, orc = dm.default_config(128), _oracle()
    sc = dm.gen_scenes(cfg, 0, 64, n_obs, junction_every=4)
    hidden, shorter = _copy(sc), _copy(sc)
    for s in range(64):
        _hide(hidden, s, n_obs - 1)
    shorter["scene_in"]["obs_n"] -= 1
    full, got, want = _run(orc, cfg, sc), _run(orc, cfg, hidden), _run(orc, cfg, shorter)
    _same(got, want, f"{n_obs} obstacles, the last one hidden against obs_n - 1")
    assert any(x.tobytes() != y.tobytes() for x, y in zip(full, want)), "the entry matters: removing it changes the outputs"


@pytest.mark.parametrize("n_obs", [8, 64])
def test_hidden_middle_entry_is_the_entry_deleted(n_obs):
    cfg, orc = dm.default_config(128), _oracle()
    sc = dm.gen_scenes(cfg, 0, 64, n_obs, junction_every=4)
    hidden, deleted = _copy(sc), _copy(sc)
    j = n_obs // 2
    for s in range(64):
        _hide(hidden, s, j)
        off = int(sc["scene_in"]["obs_off"][s])
        for pool in ("obs_pool", "mot_pool"):
            deleted[pool][off + j:off + n_obs - 1] = sc[pool][off + j + 1:off + n_obs]
    deleted["scene_in"]["obs_n"] -= 1
    # no output record carries an obstacle INDEX (PlanOut.ob and around[] are copies of the entries): every byte is compared
    _same(_run(orc, cfg, hidden), _run(orc, cfg, deleted), f"{n_obs} obstacles, entry {j} hidden against the entry deleted")

"""grl_act(GRL_ACT_GREEDY) on the MI355X: the one-launch epsilon-greedy act of the DQN / BDQ networks (csrc/q_act.h) and the
select kernel other shapes get, against the arg-max of the oracle's Q-values; the override table; ties; polling; and BDQ
learning on 8 environments through model.learn."""
import json
import os

import numpy as np
import pytest

import q_parity_util as qu
from grasp_rl import _capi, synthetic
from grasp_rl.engine import QEngine
from oracle import dqn as od
from q_parity_util import TIE_CAP, TIE_REL, compared_pairs      # noqa: F401  (shared with tests/test_gpu_q_shapes.py)

gpu = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def shipped_case(name, n):
    """The shapes the reference's command line selects: DQN [64, 64] on 100 features, BDQ [[64, 64], [32], [32]] x 33 bins on
    the 101-d observation with 5 action dimensions (seeded Xavier weights: the shipped BDQ_33pads_big network has another
    shape -- it is the `golden` case), and that shipped network itself (layers [[512, 256], [128], [128]]: select-kernel path)."""
    if name == "golden":
        sp = json.load(open(os.path.join(GOLD, "oracle_pins.json")))["bdq_real_obs"]["spec"]
        z = np.load(os.path.join(GOLD, "bdq_33_big_best_model.npz"))
        spec = od.bdq_spec(sp["obs_dim"], sp["branches"], sp["bins"], [list(sp["common"]), [sp["branch"]], [sp["value"]]])
        params = {k: z[k] for k in z.files}
    else:
        c = qu.CASES[name]
        spec = od.QSpec(algo=c["algo"], obs_dim=c["obs_dim"], n_branches=c["D"], n_bins=c["bins"], common=list(c["common"]),
                        branch_hidden=list(c["branch"]), value_hidden=list(c["value"]))
        params = od.init_params(spec, seed=11)
        rng = np.random.default_rng(12)
        for k in params:          # biases away from zero: the value tower and every bias add take part
            if k.endswith("biases:0"):
                params[k] = rng.uniform(-0.1, 0.1, params[k].shape).astype(np.float32)
    cfg = _capi.make_q_config(spec.algo, spec.obs_dim, spec.n_branches, spec.n_bins, tuple(spec.common), tuple(spec.branch_hidden),
                              tuple(spec.value_hidden), batch_size=8, act_batch=n, replay_capacity=16)
    obs = np.random.default_rng(100 + n).normal(0.0, 1.0, (n, spec.obs_dim)).astype(np.float32)
    return spec, params, cfg, obs


def test_tie_cap_holds_for_the_oracle_alone():
    """CPU part of the cases below: with these seeds the oracle itself leaves at most 5 % of the pairs of every case out."""
    for name in ("dqn_reference_shape", "bdq_baseline_config3", "golden"):
        for n in (1, 16, 64):
            spec, params, _, obs = shipped_case(name, n)
            keep = compared_pairs(od.QOracle(spec, params).q_values(obs))
            assert keep.any() and (~keep).mean() <= TIE_CAP, (name, n, (~keep).mean())
    for name in qu.SHAPE_CASES:          # ... and of the boundary shapes (tests/test_gpu_q_shapes.py)
        for n in qu.ACT_NS:
            spec, params, _, obs = qu.act_case(name, n)
            keep = compared_pairs(od.QOracle(spec, params).q_values(obs))
            assert keep.any() and (~keep).mean() <= TIE_CAP, (name, n, (~keep).mean())


@gpu
@pytest.mark.parametrize("n", [1, 16, 64])
@pytest.mark.parametrize("name,fused", [("dqn_reference_shape", True), ("bdq_baseline_config3", True), ("golden", False)])
def test_bins_equal_the_argmax_of_the_oracle(name, fused, n, capfd, monkeypatch):
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    spec, params, cfg, obs = shipped_case(name, n)
    q = od.QOracle(spec, params).q_values(obs)
    keep = compared_pairs(q)
    assert keep.any() and (~keep).mean() <= TIE_CAP, (~keep).mean()
    eng = QEngine(cfg)
    try:
        plan = capfd.readouterr().err
        assert ("epsilon-greedy act: one launch" in plan) == fused, plan
        eng.set_parameters(params)
        bins = eng.act_bins(obs)
        assert bins.shape == (n, spec.n_branches) and bins.dtype == np.int64
        want = q.argmax(axis=2)
        print("%s n=%d: %d of %d pairs compared, %d differ" % (name, n, keep.sum(), keep.size, (bins != want)[keep].sum()))
        assert np.array_equal(bins[keep], want[keep])
        assert np.array_equal(eng.act_bins(obs[:1]), bins[:1])                  # fewer rows than act_batch
        assert np.array_equal(eng.act_bins(obs), bins)                           # and again: the completion counter keeps step
        # the Q-value path is what it was: same arg-max wherever ITS top two are apart, and untouched by the greedy calls between
        qd = eng.q_values(obs)
        assert np.array_equal(qd.argmax(axis=2)[keep], want[keep])
        assert np.array_equal(eng.q_values(obs), qd)
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("name", ["dqn_reference_shape", "bdq_baseline_config3", "golden"])
def test_override_and_ties(name):
    n = 16
    spec, params, cfg, obs = shipped_case(name, n)
    D, nb = spec.n_branches, spec.n_bins
    eng = QEngine(cfg)
    try:
        eng.set_parameters(params)
        greedy = eng.act_bins(obs)
        rng = np.random.default_rng(1)
        explore = np.where(rng.random((n, D)) < 0.5, rng.integers(0, nb, (n, D)), -1)
        explore[0], explore[1] = -1, np.arange(D) % nb              # an all-greedy row, an all-explored row
        got = eng.act_bins(obs, explore)
        assert np.array_equal(got, np.where(explore >= 0, explore, greedy))
        assert np.array_equal(eng.act_bins(obs, np.full((n, D), -1)), greedy)
        # an exact tie built on purpose: two equal columns of every branch's output layer (kernel and bias) that beat all
        # others -- the lower index wins, as np.argmax has it
        lo, hi = 2, nb - 3
        tied = dict(params)
        outs = [k for k in params if "/target_q_func/" not in k and "/action_value/" in k and k.endswith("weights:0") and params[k].shape[1] == nb]
        outs = outs if spec.algo == "bdq" else outs[-1:]
        assert len(outs) == D
        for k in outs:
            w, b = np.array(params[k]), np.array(params[k.replace("weights:0", "biases:0")])
            w[:, hi] = w[:, lo]
            b[lo] = b[hi] = 50.0
            tied[k], tied[k.replace("weights:0", "biases:0")] = w, b
        eng.set_parameters(tied)
        assert np.array_equal(eng.act_bins(obs), np.full((n, D), lo))
        qt = eng.q_values(obs)
        assert np.array_equal(qt[:, :, lo], qt[:, :, hi]) and np.array_equal(qt.argmax(axis=2), np.full((n, D), lo))
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("tune", ["act_poll=0", "q_act=0", "q_act=0,act_poll=0"])
def test_routing_switches_give_the_same_bins(tune, monkeypatch):
    """GRL_TUNE act_poll=0 (synchronise the stream instead of polling) and q_act=0 (launch list of the Q-value path + select
    kernel) return the bins of the default path; the Q-values of a handle that never ran the new kernel equal, byte for byte,
    those of one that did."""
    spec, params, cfg, obs = shipped_case("bdq_baseline_config3", 16)
    keep = compared_pairs(od.QOracle(spec, params).q_values(obs))

    def run():
        eng = QEngine(cfg)
        try:
            eng.set_parameters(params)
            explore = np.where(np.arange(16 * spec.n_branches).reshape(16, -1) % 3 == 0, 7, -1)
            return eng.act_bins(obs), eng.act_bins(obs, explore), eng.q_values(obs)
        finally:
            eng.close()
    base = run()
    monkeypatch.setenv("GRL_TUNE", tune)
    other = run()
    if "q_act=0" in tune:         # another summation order: equal wherever the top two are apart
        assert np.array_equal(base[0][keep], other[0][keep]) and np.array_equal(base[1][keep], other[1][keep])
    else:
        assert np.array_equal(base[0], other[0]) and np.array_equal(base[1], other[1])
    assert base[2].tobytes() == other[2].tobytes()


@gpu
def test_greedy_flag_is_refused_on_sac_handles():
    import parity_util as pu
    from grasp_rl._capi import GrlError
    eng = pu.engine_setup(pu.make_case(extractor="augmented", kind="depth", B=8, n_replay=32, n_steps=1))
    try:
        obs = np.zeros((1, 64, 64, eng.cfg.obs_channels), np.float32)
        out = np.zeros((1, eng.A), np.float32)
        rc = eng.lib.grl_act(eng.h, obs.ctypes.data, 1, _capi.ACT_GREEDY | _capi.ACT_DETERMINISTIC, None, out.ctypes.data)
        assert rc == -3, rc        # GRL_ERR_STATE
        with pytest.raises(GrlError):
            _capi.check(eng.lib, rc)
    finally:
        eng.close()


@gpu
def test_bdq_with_prioritised_replay_learns_on_eight_environments():
    """test_bdq_with_prioritised_replay_learns (tests/test_gpu_learning.py) on 8 ReachGraspEnvs: the same update budget -- one
    update per environment step, 80 000 of them -- and that test's bar (random: 0.07)."""
    r = synthetic.learn_reach("bdq", "vector", total_timesteps=80_000, q_envs=8)
    print(r)
    assert all(np.isfinite(v) for v in r["metrics"].values())
    assert r["env_steps"] == 80_000 and r["updates"] >= 78_000
    assert r["eval_success"] >= 0.8, r

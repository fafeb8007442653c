"""Layer-normalised DQN / BDQ (LnMlpPolicy, policy_kwargs layer_norm=True) on the CPU through the TEST-ONLY emulation build:
the launch plan of csrc/plan_q.inl with the sequential reference forms of csrc/ln_kernels.h (tests/hostemu/ln_kernels_ref1.h)
against the float64 restatement of tests/q_layer_norm_util.py -- which is itself held against oracle/dqn.py first.  The kernels
themselves are tests/test_gpu_q_layer_norm.py's."""
import os

import numpy as np
import pytest
import torch

import q_layer_norm_util as lu
import q_parity_util as qu
from fake_env import FakeGraspEnv
import stable_baselines as sb
from grasp_rl import _capi
from grasp_rl.engine import QEngine
from grasp_rl.sb.dqn import BDQ, DQN
from grasp_rl.sb.vec_env import DummyVecEnv
from hostemu_backend import NumpyHostBackend
from oracle import dqn as od
from stable_baselines.bdq.policies import MlpActPolicy
from stable_baselines.deepq.policies import LnMlpPolicy, MlpPolicy

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LN_LINE = "grl plan: q layer_norm   per-layer launches + ln_relu_fwd/bwd"


# ------------------------------------------------------------------------------------------ the reference, before it is used
class _Oracle64(od.QOracle):
    """oracle/dqn.py's own update, every tensor float64"""
    def tensors(self, grad=False):
        T = super().tensors(grad=False)
        out = {}
        for k, t in T.items():
            out[k] = torch.from_numpy(np.asarray(self.P[k], np.float64).copy())
            if grad and k in self.train_names:
                out[k].requires_grad_(True)
        return out


@pytest.mark.parametrize("name", ["dqn", "bdq"])
def test_restatement_agrees_with_the_oracle_without_layer_norm(name):
    case = qu.make_q_case(**qu.CASES[name])
    spec = case["spec"]
    params = lu.init_ln_params(spec, 3, layer_norm=False)
    assert list(params) == list(od.param_shapes(spec))
    ref = lu.QRef64(spec, params, layer_norm=False)
    tr, ii = case["tr"], case["idx"][0]
    batch = {k: tr[k][ii] for k in ("obs", "next_obs", "act", "rew", "done")}
    out = ref.grads(batch, case["weights"][0])
    o64 = _Oracle64(spec, params)
    want, G = o64.grads({k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in batch.items()}, case["weights"][0])
    # float64 against float64: a few ulp of the operands
    assert np.abs(out["td"] - want["td"]).max() <= 1e-12 * max(1.0, np.abs(want["td"]).max())
    assert abs(out["loss"] - want["loss"]) <= 1e-12 * abs(want["loss"])
    for n, g in G.items():
        assert np.abs(out["grads"][n] - g).max() <= 1e-12 * max(np.abs(g).max(), 1e-30), n
    assert np.abs(ref.q_values(batch["obs"]) - want["q"]).max() <= 1e-12 * np.abs(want["q"]).max()
    # clip_by_norm + Adam against the oracle's float32 step on the same minibatch: float32 rounding of one step
    f32 = od.QOracle(spec, params)
    f32.step({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in batch.items()}, case["weights"][0])
    ref.step(batch, case["weights"][0])
    for n in ref.train_names:
        assert np.abs(ref.P64[n] - f32.P[n]).max() <= 1e-6, n


def test_seeds_leave_no_sign_ambiguous_unit_and_no_act_tie():
    for name in lu.LN_CASES:
        case = lu.make_ln_case(name)
        steps, _ = lu.reference_run(case)
        lu.assert_no_sign_ambiguity(steps)
        assert all(lu._act_gap_ok(case, n) for n in qu.ACT_NS), name


# ------------------------------------------------------------------------------------------ C ABI, emulation build
@pytest.mark.parametrize("name", list(lu.LN_CASES))
def test_update_matches_the_float64_reference(hostemu_lib, name, monkeypatch, capfd):
    """forward, every gradient tensor (gamma / beta included), one optimiser step on identical inputs, three updates, target copy"""
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    lu.run_and_compare_ln(lu.make_ln_case(name), backend=NumpyHostBackend(), lib_path=hostemu_lib)
    plan = capfd.readouterr().err
    assert LN_LINE in plan
    # no chains, no chained backward, no four-launch multi-update calls, no one-launch act
    assert "grl plan: q chains" not in plan and "inside the backward chains" not in plan and "grl plan: q_pf " not in plan
    assert "sampler on the apply launch): yes" not in plan
    assert "+ select kernel" in plan and "act: one launch" not in plan


def test_switches_do_not_move_a_layer_norm_handle_off_its_route(hostemu_lib, monkeypatch, capfd):
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    monkeypatch.setenv("GRL_TUNE", "fused_q=1,q_chain=1,q_act=1,q_pf=1,per_pf=1")
    lu.run_and_compare_ln(lu.make_ln_case("dqn_48"), backend=NumpyHostBackend(), lib_path=hostemu_lib)
    plan = capfd.readouterr().err
    assert LN_LINE in plan and "grl plan: q chains" not in plan and "act: one launch" not in plan


@pytest.mark.parametrize("name", ["dqn_64_64", "bdq_shipped"])
def test_variable_table(hostemu_lib, name):
    case = lu.make_ln_case(name)
    eng = QEngine(case["cfg"], backend=NumpyHostBackend(), lib_path=hostemu_lib)
    try:
        names = [t[0] for t in eng.table]
        shapes = {t[0]: tuple(t[3]) for t in eng.table}
    finally:
        eng.close()
    if name == "dqn_64_64":
        pre = "deepq/model/action_value/"
        assert names[:9] == ["deepq/eps:0", pre + "fully_connected/weights:0", pre + "fully_connected/biases:0",
                             pre + "LayerNorm/beta:0", pre + "LayerNorm/gamma:0", pre + "fully_connected_1/weights:0",
                             pre + "fully_connected_1/biases:0", pre + "LayerNorm_1/beta:0", pre + "LayerNorm_1/gamma:0"]
        assert names[9:11] == [pre + "fully_connected_2/weights:0", pre + "fully_connected_2/biases:0"]      # output layer: none
        assert names[11:15] == ["deepq/model/state_value/fully_connected/weights:0", "deepq/model/state_value/fully_connected/biases:0",
                                "deepq/model/state_value/LayerNorm/beta:0", "deepq/model/state_value/LayerNorm/gamma:0"]
        assert shapes[pre + "LayerNorm_1/gamma:0"] == (64,)
        assert "deepq/target_q_func/model/state_value/LayerNorm_1/gamma:0" in names
    else:
        pre = "bdq/model/"
        assert names[1:9] == [pre + "common_net/fully_connected/weights:0", pre + "common_net/fully_connected/biases:0",
                              pre + "common_net/LayerNorm/beta:0", pre + "common_net/LayerNorm/gamma:0",
                              pre + "common_net/fully_connected_1/weights:0", pre + "common_net/fully_connected_1/biases:0",
                              pre + "common_net/LayerNorm_1/beta:0", pre + "common_net/LayerNorm_1/gamma:0"]
        # four branches share the action_value scope: LayerNorm, LayerNorm_1 .. _3 behind fully_connected, _2, _4, _6
        for br in range(4):
            k = names.index(pre + "action_value/" + od._fc(2 * br) + "/biases:0")
            assert names[k + 1:k + 3] == [pre + "action_value/%s/beta:0" % lu._ln(br), pre + "action_value/%s/gamma:0" % lu._ln(br)]
        assert shapes[pre + "common_net/LayerNorm/beta:0"] == (512,) and shapes[pre + "action_value/LayerNorm_3/gamma:0"] == (128,)
        assert sum("LayerNorm" in n for n in names) == 2 * 2 * (2 + 4 + 1)
    assert names == list(lu.ln_param_shapes(case["spec"]))


@pytest.mark.parametrize("prioritised", [False, True])
def test_multi_update_call_equals_single_calls(hostemu_lib, prioritised):
    lu.multi_update_check("bdq_no_trunk", prioritised, backend=NumpyHostBackend(), lib_path=hostemu_lib)
    lu.multi_update_check("dqn_48", prioritised, backend=NumpyHostBackend(), lib_path=hostemu_lib)


@pytest.mark.parametrize("n", [1, 17])
def test_act_bins(hostemu_lib, n):
    lu.act_check(lu.make_ln_case("bdq_no_trunk"), n, backend=NumpyHostBackend(), lib_path=hostemu_lib)
    lu.act_check(lu.make_ln_case("dqn_100_65"), n, backend=NumpyHostBackend(), lib_path=hostemu_lib)


def test_plan_without_layer_norm_is_the_parent_commits(hostemu_lib, monkeypatch, capfd):
    """tests/golden/q_plan_dump_parent.txt: GRL_PLAN_DUMP of q_layer_norm = 0 handles, captured from the commit before the
    field existed -- chains, per-layer launches (by shape and by switch), both apply forms."""
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    text = open(os.path.join(GOLD, "q_plan_dump_parent.txt")).read()
    sections = [s for s in text.split("== ") if s]
    assert len(sections) == 6
    for sec in sections:
        head, want = sec.split("\n", 1)
        name, tune = head.split(" GRL_TUNE=")
        monkeypatch.setenv("GRL_TUNE", tune)
        capfd.readouterr()
        case = qu.make_q_case(**qu.case_args(name))
        assert case["cfg"].q_layer_norm == 0
        QEngine(case["cfg"], backend=NumpyHostBackend(), lib_path=hostemu_lib).close()
        assert capfd.readouterr().err == want, head


def test_plans_tables_and_arena_sizes_are_the_parent_commits(hostemu_lib, monkeypatch, capfd):
    """tests/golden/q_plan_parent_routes.json (tests/q_plan_routes_util.py): the plan dump, the variable table and the arena
    sizes of every shape / layer-norm / wide case, two prioritised handles and the baseline shape with each route switch off,
    captured from the commit before plan_q became a list of steps over one tower list."""
    import q_plan_routes_util as ru
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    gold = ru.load_golden(os.path.join(GOLD, "q_plan_parent_routes.json"))
    cases = ru.route_cases()
    assert [c[0] for c in cases] == list(gold)
    for cid, tune, make in cases:
        want = gold[cid]
        assert want["tune"] == tune
        monkeypatch.setenv("GRL_TUNE", tune) if tune else monkeypatch.delenv("GRL_TUNE", raising=False)
        got = ru.snapshot(make(), lambda: capfd.readouterr().err, hostemu_lib)
        assert got["plan"] == want["plan"], cid
        assert got["table"] == want["table"], cid
        assert got["sizes"] == want["sizes"], cid


def test_state_checkpoint_round_trip_and_refusal(hostemu_lib, tmp_path):
    case = lu.make_ln_case("bdq_no_trunk", n_replay=60)
    a = lu.engine_setup(case, NumpyHostBackend(), hostemu_lib)
    b = lu.engine_setup(lu.make_ln_case("bdq_no_trunk", n_replay=60), NumpyHostBackend(), hostemu_lib)
    plain = lu.make_ln_case("bdq_no_trunk", n_replay=60, layer_norm=False)
    c = lu.engine_setup(plain, NumpyHostBackend(), hostemu_lib)
    try:
        a.train_device(3)
        c.train_device(1)
        a.save_state(str(tmp_path / "ln"))
        c.save_state(str(tmp_path / "plain"))
        b.load_state(str(tmp_path / "ln"))
        Pa, Pb = a.get_parameters(), b.get_parameters()
        ln_names = [n for n in Pa if "LayerNorm" in n and "/target_q_func/" not in n]
        assert ln_names and all(not np.array_equal(Pa[n], case["params"][n]) for n in ln_names)
        assert all(np.array_equal(Pa[n], Pb[n]) for n in Pa)
        for what in ("adam_m", "adam_v"):
            assert np.array_equal(a.fetch(what), b.fetch(what)) and np.abs(a.fetch(what)).max() > 0
        a.train_device(2)
        b.train_device(2)
        Pa, Pb = a.get_parameters(), b.get_parameters()
        assert all(np.array_equal(Pa[n], Pb[n]) for n in Pa)
        before = b.get_parameters()
        with pytest.raises(_capi.GrlError):
            b.load_state(str(tmp_path / "plain"))          # saved without layer norm: refused by a layer-norm handle
        after = b.get_parameters()
        assert all(np.array_equal(before[n], after[n]) for n in before)
    finally:
        for e in (a, b, c):
            e.close()


# ------------------------------------------------------------------------------------------ model level
@pytest.fixture
def emulated_q_engine(hostemu_lib, monkeypatch):
    f = staticmethod(lambda cfg, device: QEngine(cfg, backend=NumpyHostBackend(), lib_path=hostemu_lib))
    monkeypatch.setattr(DQN, "_engine_factory", f)
    monkeypatch.setattr(BDQ, "_engine_factory", f)


def _models():
    dqn_env = lambda s=0: DummyVecEnv([lambda: FakeGraspEnv(seed=s, vector_dim=20, discrete_actions=6)])
    bdq_env = lambda s=0: DummyVecEnv([lambda: FakeGraspEnv(seed=s, vector_dim=20, act_dim=3)])
    return [
        (lambda: sb.DQN(LnMlpPolicy, dqn_env(), batch_size=8, learning_starts=10, target_network_update_freq=10, buffer_size=64,
                        policy_kwargs={"layers": [24, 16]}), dqn_env),
        (lambda: sb.DQN(MlpPolicy, dqn_env(), batch_size=8, learning_starts=10, target_network_update_freq=10, buffer_size=64,
                        policy_kwargs={"layers": [24, 16], "layer_norm": True}), dqn_env),
        (lambda: sb.BDQ(MlpActPolicy, bdq_env(), policy_kwargs={"layer_norm": True, "layers": [[16, 16], [8], [8]]}, batch_size=8,
                        buffer_size=64, num_actions_pad=5, learning_starts=10, target_network_update_freq=10), bdq_env),
    ]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_models_build_learn_save_and_load(tmp_path, emulated_q_engine, which):
    make, make_env = _models()[which]
    model = make()
    assert model.layer_norm and model.engine.cfg.q_layer_norm == 1
    P0 = model.get_parameters()
    gam = [k for k in P0 if k.endswith("/gamma:0")]
    bet = [k for k in P0 if k.endswith("/beta:0")]
    assert gam and len(gam) == len(bet)
    assert all((P0[k] == 1).all() for k in gam) and all((P0[k] == 0).all() for k in bet)
    obs = make_env(1).reset()
    a0, _ = model.predict(obs, deterministic=True)
    model.learn(total_timesteps=40)
    P1 = model.get_parameters()
    online = lambda ks: [k for k in ks if "/target_q_func/" not in k]
    assert all(not np.array_equal(P1[k], P0[k]) for k in online(gam) + online(bet))          # they are trained
    assert all(np.array_equal(P1[k], P1[k.replace("/target_q_func", "")]) for k in P1 if "/target_q_func/" in k)   # copied at step 40
    path = os.path.join(str(tmp_path), "m")
    model.save(path)
    from grasp_rl.sb import save_util
    data, _ = save_util.load_from_zip(path)
    assert data["policy_kwargs"]["layer_norm"] is True
    agent = type(model).load(path)
    assert agent.layer_norm and agent.engine.cfg.q_layer_norm == 1
    P2 = agent.get_parameters()
    assert list(P2) == list(P1) and all(np.array_equal(P1[k], P2[k]) for k in P1)
    assert np.array_equal(np.asarray(agent.predict(obs, deterministic=True)[0]), np.asarray(model.predict(obs, deterministic=True)[0]))
    # sb_helper.load_params: a subset, exact_match=False
    usable = {k: v for k, v in P1.items() if "action_value" not in k and "2" not in k}
    assert any("LayerNorm" in k for k in usable) and len(usable) < len(P1)
    fresh = make()
    fresh.load_parameters(usable, exact_match=False)
    Pf = fresh.get_parameters()
    assert all(np.array_equal(Pf[k], v) for k, v in usable.items())
    assert any(not np.array_equal(Pf[k], P1[k]) for k in P1 if k not in usable)


def test_param_noise_is_still_refused(emulated_q_engine):
    env = DummyVecEnv([lambda: FakeGraspEnv(seed=0, vector_dim=20, discrete_actions=6)])
    with pytest.raises(NotImplementedError):
        sb.DQN(LnMlpPolicy, env, param_noise=True)

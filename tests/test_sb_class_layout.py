"""The class layout of ``grasp_rl.sb``: one ``BaseModel`` under all five models, ``PPO2`` and ``TRPO`` as siblings under
``OnPolicyModel``, every shared method written once and found on the base that owns it, and the ``_net_arch`` refusals carrying
the name of the class that raised them.  No engine is built."""
import pytest

from grasp_rl import _capi
from grasp_rl.sb import on_policy
from grasp_rl.sb.base import BaseModel
from grasp_rl.sb.dqn import BDQ, DQN
from grasp_rl.sb.on_policy import OnPolicyModel
from grasp_rl.sb.ppo2 import PPO2
from grasp_rl.sb.sac import SAC
from grasp_rl.sb.trpo import TRPO
from stable_baselines.common.policies import CnnPolicy

ALL = (SAC, DQN, BDQ, PPO2, TRPO)

# method -> the classes that deliberately carry their own
BASE_METHODS = {
    "get_env": (), "get_vec_normalize_env": (), "_dp_runtime": (), "get_parameter_list": (), "get_parameters": (),
    "_learning_rate_value": (), "_begin_learn": (), "_finish_load": (),
    "load_parameters": (TRPO,),         # drops oldpi/* and calls up
    "pretrain": (SAC,),                 # the real one
    "set_env": (SAC,),                  # clears its statistics stamp and calls up
    "_training_env": (TRPO,),           # one environment, no fan-out
    "_check_fits_engine": (PPO2,),      # exactly the plan's number of environments
}
ON_POLICY_METHODS = {
    "_net_arch": (), "_check_spaces": (), "_clip": (), "predict": (), "_learn": (), "_resolve_device_norm": (),
    "_attach_device_norm": (), "_detach_device_norm": (), "_rows": (), "_loop_snapshot": (), "_resumed_start": (),
    "_host_state": (), "_restore_host_state": (),
    "_host_extra": (TRPO,), "_set_host_extra": (TRPO,),     # episode statistics and oldpi/*
    "_before_setup": (PPO2,),                               # the saved number of environments, then calls up
}


def test_trpo_and_ppo2_are_siblings():
    assert not issubclass(TRPO, PPO2) and not issubclass(PPO2, TRPO)
    assert issubclass(PPO2, OnPolicyModel) and issubclass(TRPO, OnPolicyModel)
    assert all(issubclass(cls, BaseModel) for cls in ALL)
    assert not issubclass(SAC, OnPolicyModel) and not issubclass(DQN, OnPolicyModel)


def test_trpo_carries_nothing_of_ppo2():
    assert not hasattr(TRPO, "loss_names") and not hasattr(TRPO, "_write_summary")
    assert hasattr(PPO2, "loss_names") and hasattr(PPO2, "_write_summary")
    assert not any(hasattr(cls, "_on_policy") for cls in ALL)


@pytest.mark.parametrize("name", sorted(BASE_METHODS))
def test_shared_methods_live_on_base_model(name):
    for cls in ALL:
        owner = getattr(cls, name).__qualname__.split(".")[0]
        if cls in BASE_METHODS[name]:
            assert owner == cls.__name__, (cls, name, owner)
        else:
            assert owner == "BaseModel", (cls, name, owner)


@pytest.mark.parametrize("name", sorted(ON_POLICY_METHODS))
def test_on_policy_methods_live_on_on_policy_model(name):
    for cls in (PPO2, TRPO):
        owner = getattr(cls, name).__qualname__.split(".")[0]
        if cls in ON_POLICY_METHODS[name]:
            assert owner == cls.__name__, (cls, name, owner)
        else:
            assert owner == "OnPolicyModel", (cls, name, owner)


def test_every_model_keeps_its_own_engine_factory_and_learn():
    for cls in ALL:
        owner = DQN.__mro__[1] if cls in (DQN, BDQ) else cls      # (DQN and BDQ share _QModel's)
        assert "_engine_factory" in vars(owner) and isinstance(vars(owner)["_engine_factory"], staticmethod)
        assert cls.learn.__qualname__.split(".")[0] == owner.__name__


def test_on_policy_helpers_exist_once():
    import grasp_rl.sb.ppo2 as ppo2
    import grasp_rl.sb.trpo as trpo
    for name in ("_episodes", "_safe_mean", "explained_variance", "_normalize_kwargs"):
        assert getattr(on_policy, name).__module__ == "grasp_rl.sb.on_policy"
        for mod in (ppo2, trpo):
            assert getattr(mod, name, getattr(on_policy, name)) is getattr(on_policy, name)


def relu(x):
    return x


L = _capi.GRL_MAX_LAYERS
REFUSALS = [
    ("CnnPolicy", {}, "%s: policy 'CnnPolicy' is not implemented (only the actor-critic MlpPolicy)"),
    (CnnPolicy, {}, "%s: policy ActorCriticCnnPolicy is not implemented (only the actor-critic MlpPolicy: CnnPolicy, "
                    "MlpLstmPolicy and their relatives are refused)"),
    (type("MlpLstmPolicy", (), {}), {}, "%s: policy MlpLstmPolicy is not implemented (only the actor-critic MlpPolicy: CnnPolicy, "
                                        "MlpLstmPolicy and their relatives are refused)"),
    ("MlpPolicy", {"act_fun": relu}, "%s: act_fun relu is not implemented (the towers' activation is tanh)"),
    ("MlpPolicy", {"layers": [64], "cnn_extractor": None}, "%s: policy_kwargs ['cnn_extractor', 'layers'] are not implemented"),
    ("MlpPolicy", {"feature_extraction": "cnn"}, "%s: feature_extraction 'cnn' is not implemented"),
    ("MlpPolicy", {"net_arch": [64, dict(pi=[32], vf=[32])]},
     "%s: shared layers in net_arch are not implemented (net_arch must be [dict(vf=[...], pi=[...])], got "
     "[64, {'pi': [32], 'vf': [32]}])"),
    ("MlpPolicy", {"net_arch": [dict(pi=[], vf=[32])]}, "%%s: the pi tower needs 1..%d layers of widths 1..1024, got []" % L),
    ("MlpPolicy", {"net_arch": [dict(pi=[32], vf=[8] * (L + 1))]},
     "%%s: the vf tower needs 1..%d layers of widths 1..1024, got %r" % (L, [8] * (L + 1))),
    ("MlpPolicy", {"net_arch": [dict(pi=[32, 0], vf=[32])]}, "%%s: the pi tower needs 1..%d layers of widths 1..1024, got [32, 0]" % L),
    ("MlpPolicy", {"net_arch": [dict(pi=[32], vf=[1025])]}, "%%s: the vf tower needs 1..%d layers of widths 1..1024, got [1025]" % L),
]


@pytest.mark.parametrize("cls", (PPO2, TRPO))
@pytest.mark.parametrize("policy,kwargs,text", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_net_arch_refusals_carry_the_class_name(monkeypatch, cls, policy, kwargs, text):
    monkeypatch.delenv("GRL_DATA_PARALLEL", raising=False)
    model = cls(policy, None, policy_kwargs=kwargs, _init_setup_model=False)
    assert cls._net_arch.__qualname__ == "OnPolicyModel._net_arch"
    with pytest.raises(NotImplementedError) as e:
        model._net_arch()
    assert str(e.value) == text % cls.__name__


@pytest.mark.parametrize("cls", (PPO2, TRPO))
def test_net_arch_accepts_what_the_plan_builds(monkeypatch, cls):
    monkeypatch.delenv("GRL_DATA_PARALLEL", raising=False)
    assert cls("MlpPolicy", None, _init_setup_model=False)._net_arch() == ((64, 64), (64, 64))
    kw = {"net_arch": [dict(pi=[1, 1024], vf=[8] * L)], "act_fun": type("tanh", (), {})}
    assert cls("MlpPolicy", None, policy_kwargs=kw, _init_setup_model=False)._net_arch() == ((1, 1024), (8,) * L)

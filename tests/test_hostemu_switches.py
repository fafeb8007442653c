"""The one table of GRL_* switches (csrc/engine.hip; README.md, "Switches") on the emulation build: what GRL_PLAN_DUMP says about
the keys GRL_TUNE names -- the recognised ones off their default, the unknown ones -- and that every switch string the fallback
tests set is a key of the table (a renamed key would otherwise leave such a test passing on the default plan)."""
import re

import pytest

import parity_util as pu
import switch_util as su
import test_gpu_parity
import test_gpu_q_act
import test_gpu_q_parity
import test_hostemu_plan
import test_hostemu_q_plan
from hostemu_backend import NumpyHostBackend

SETTING = re.compile(r"GRL_[A-Z0-9_]+=\S*|[a-z0-9_]+=[^,\s]*(,[a-z0-9_]+=[^,\s]*)*")


def switch_strings():
    """Every parametrised value of the five test modules that sets a switch: `GRL_X=...` or a GRL_TUNE string."""
    found = []
    for mod in (test_gpu_parity, test_gpu_q_parity, test_gpu_q_act, test_hostemu_plan, test_hostemu_q_plan):
        for fn in vars(mod).values():
            for mark in getattr(fn, "pytestmark", None) or []:
                if mark.name != "parametrize":
                    continue
                for value in mark.args[1]:
                    for s in value if isinstance(value, (tuple, list)) else (value,):
                        if isinstance(s, str) and SETTING.fullmatch(s) and s not in found:
                            found.append(s)
    return found


SWITCH_STRINGS = switch_strings()


def test_the_collection_sees_every_module_that_parametrises_switches():
    for s in ("GRL_NO_V2=1", "GRL_TUNE=conv_stack_bwd=1", "GRL_NO_HEADS_MFMA=1", "q_chain_late=0", "q_act=0,act_poll=0"):
        assert s in SWITCH_STRINGS, SWITCH_STRINGS


def sac_dump(monkeypatch, capfd, env, kw, hostemu_lib):
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    monkeypatch.setenv(*env)
    capfd.readouterr()
    case = pu.make_case(n_steps=1, **kw)
    pu.SacEngine(case["cfg"], backend=NumpyHostBackend(), lib_path=hostemu_lib).close()
    return capfd.readouterr().err


def test_known_unknown_and_prefix_keys_dqn(hostemu_lib, monkeypatch, capfd):
    su.check_mixed_string(lambda tune: su.dqn_dump(monkeypatch, capfd, tune, NumpyHostBackend(), hostemu_lib), matrix_cores=False)


def test_known_and_unknown_keys_sac_mlp(hostemu_lib, monkeypatch, capfd):
    dump = sac_dump(monkeypatch, capfd, ("GRL_TUNE", su.MIXED), test_hostemu_plan.CASES["mlp_features"], hostemu_lib)
    settings, unknown = su.tune_notes(dump)
    assert len(settings) >= 1 and all(s == ["fused_qapply=0", "q_chain_late=0"] for s in settings), dump
    assert unknown == ["bogus"] * len(settings), dump


@pytest.mark.parametrize("tune", ["q_chain=0,q_chain_late=0,wg_split=72/12/6,dp_blocks=64/32/16",
                                  "dp_blocks=64/32/16,q_chain_late=0,wg_split=72/12/6,q_chain=0"])
def test_prefix_keys_and_triples_parse_to_their_own_rows(hostemu_lib, monkeypatch, capfd, tune):
    for dump in (su.dqn_dump(monkeypatch, capfd, tune, NumpyHostBackend(), hostemu_lib),
                 sac_dump(monkeypatch, capfd, ("GRL_TUNE", tune), test_hostemu_plan.CASES["mlp_features"], hostemu_lib)):
        settings, unknown = su.tune_notes(dump)
        assert len(settings) >= 1 and all(s == sorted(tune.split(",")) for s in settings) and unknown == [], dump
    # ... and `q_chain_late=0` alone names no `q_chain` (the route side of it: switch_util.check_mixed_string)
    settings, _ = su.tune_notes(su.dqn_dump(monkeypatch, capfd, "q_chain_late=0", NumpyHostBackend(), hostemu_lib))
    assert all(s == ["q_chain_late=0"] for s in settings)


@pytest.mark.parametrize("setting", SWITCH_STRINGS)
def test_switch_strings_of_the_fallback_tests_are_keys_of_the_table(hostemu_lib, monkeypatch, capfd, setting):
    """Under each string a SAC handle (the CNN configuration the SAC fallback tests run) and a DQN handle are created: no
    unknown-key line, and every `key=value` of the string on the `grl tune:` line (all of them are off their default)."""
    env = tuple(setting.split("=", 1)) if setting.startswith("GRL_") else ("GRL_TUNE", setting)
    want = env[1].split(",") if env[0] == "GRL_TUNE" else [setting]
    dumps = [sac_dump(monkeypatch, capfd, env, test_hostemu_plan.CASES["depth_augmented"], hostemu_lib),
             su.dqn_dump(monkeypatch, capfd, env[1] if env[0] == "GRL_TUNE" else "", NumpyHostBackend(), hostemu_lib)]
    for dump in dumps:
        settings, unknown = su.tune_notes(dump)
        assert unknown == [] and len(settings) >= 1, dump
        for s in settings:
            assert set(want) <= set(s), (want, s)

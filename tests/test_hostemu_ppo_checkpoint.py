"""grl_ppo_state_size / _export / _import and PpoEngine / TrpoEngine.save_state / load_state on the g++ emulation build
(tests/ppo_checkpoint_util.py; tests/test_gpu_ppo_checkpoint.py runs the same functions on the MI355X).  Shapes: PPO n_envs 3,
n_steps 4, towers [16] / [8, 8], minibatch 6, normalize 0 and 2; TRPO n_steps 8, vf_batch 4, cg_iters 3.  Equality of raw words
throughout."""
import ctypes as C
import os

import pytest

import ppo_checkpoint_util as cu
from hostemu_backend import NumpyHostBackend


@pytest.fixture(scope="module")
def emu(hostemu_lib):
    os.environ.pop("GRL_TUNE", None)
    return hostemu_lib


def _engine(emu, kind, normalize=0, **over):
    return cu.make_engine(kind, NumpyHostBackend, emu, normalize=normalize, **over)


@pytest.mark.parametrize("position", ["empty", "open", "closed"])
@pytest.mark.parametrize("case", sorted(cu.ENGINE_CASES))
def test_imported_handle_continues_bit_identically(emu, case, position):
    cu.check_continuation(case, position, NumpyHostBackend, emu)


def test_export_after_an_odd_number_of_observe_calls(emu):
    cu.check_statistics_parity("ppo", NumpyHostBackend, emu)


@pytest.mark.parametrize("kind", ["ppo", "trpo"])
def test_every_refusal_is_raised_by_name_and_changes_nothing(emu, kind):
    cu.check_refusals(kind, NumpyHostBackend, emu)


def test_other_handles_refuse_the_three_calls(emu):
    cu.check_other_handles(NumpyHostBackend, emu)


def test_generic_state_calls_stay_refused_on_rollout_handles(emu):
    for kind in ("ppo", "trpo"):
        eng = _engine(emu, kind)
        assert eng.lib.grl_state_size(eng.h, C.byref(C.c_size_t())) == -3
        assert eng.lib.grl_replay_segments(eng.h, 0, None) == -3
        eng.close()


@pytest.mark.parametrize("kind,normalize", [("ppo", 0), ("ppo", 2), ("trpo", 0)])
@pytest.mark.parametrize("include_replay", [True, False], ids=["with_rollout", "without_rollout"])
def test_save_state_and_load_state(emu, tmp_path, kind, normalize, include_replay):
    cu.check_save_and_load(kind, normalize, include_replay, NumpyHostBackend, emu, str(tmp_path / "ck"))
    assert sorted(os.listdir(tmp_path)) == ["ck"]            # no .tmp / .old left behind


def test_load_state_checks_before_it_overwrites(emu, tmp_path):
    cu.check_load_state_checks_first(NumpyHostBackend, emu, tmp_path)


def test_interrupted_save_leaves_the_previous_checkpoint(emu, tmp_path, monkeypatch):
    """os.rename fails once, between the two renames: load_state finds the previous checkpoint at <dir>.old."""
    cu.check_interrupted_save(NumpyHostBackend, emu, tmp_path, monkeypatch)

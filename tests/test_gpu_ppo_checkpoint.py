"""grl_ppo_state_size / _export / _import and PpoEngine / TrpoEngine.save_state / load_state on the MI355X (real library,
TorchCudaBackend with the page-locked staging of save_state / load_state): the functions of tests/ppo_checkpoint_util.py that
tests/test_hostemu_ppo_checkpoint.py runs on the emulation build, at the same shapes.  Equality of raw words throughout."""
import os

import pytest

import ppo_checkpoint_util as cu
from grasp_rl.engine import TorchCudaBackend

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def no_tune(monkeypatch):
    monkeypatch.delenv("GRL_TUNE", raising=False)


@pytest.mark.parametrize("position", ["empty", "open", "closed"])
@pytest.mark.parametrize("case", sorted(cu.ENGINE_CASES))
def test_imported_handle_continues_bit_identically(case, position):
    cu.check_continuation(case, position, TorchCudaBackend, None)


def test_export_after_an_odd_number_of_observe_calls():
    cu.check_statistics_parity("ppo", TorchCudaBackend, None)


@pytest.mark.parametrize("kind", ["ppo", "trpo"])
def test_every_refusal_is_raised_by_name_and_changes_nothing(kind):
    cu.check_refusals(kind, TorchCudaBackend, None)


def test_other_handles_refuse_the_three_calls():
    cu.check_other_handles(TorchCudaBackend, None)


@pytest.mark.parametrize("kind,normalize", [("ppo", 0), ("ppo", 2), ("trpo", 0)])
@pytest.mark.parametrize("include_replay", [True, False], ids=["with_rollout", "without_rollout"])
def test_save_state_and_load_state(tmp_path, kind, normalize, include_replay):
    cu.check_save_and_load(kind, normalize, include_replay, TorchCudaBackend, None, str(tmp_path / "ck"))
    assert sorted(os.listdir(tmp_path)) == ["ck"]            # no .tmp / .old left behind


def test_load_state_checks_before_it_overwrites(tmp_path):
    cu.check_load_state_checks_first(TorchCudaBackend, None, tmp_path)


def test_interrupted_save_leaves_the_previous_checkpoint(tmp_path, monkeypatch):
    cu.check_interrupted_save(TorchCudaBackend, None, tmp_path, monkeypatch)
